// The label solver of libphmrf (phmrf_mrf_solve and its pieces, include/phmrf.h): the coarse child problems, one round of
// every move type, the schedule between the rounds.  Host code only: the moves' kernels are in the other .hip files.

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>

#include "common.h"

namespace phmrf {

// ---- coarse alpha-expansions (coarse.hip) ----------------------------------------------------------------------
static const int COARSE_SCALE[N_COARSE] = {2, 4, 8};
// a child problem has two labels, keep = 0 and switch = 1: its strip passes are expansions of label 1 and count as such, in the
// child's own bank (where strip_kernel then finds the bank's trace counters)
static const int COARSE_CHILD_SLOT = COUNTER_EXPANSION + 1;
static const int GEOM_R[3] = {0, 2, 4}, GEOM_C[3] = {0, 21, 42};
// the schedule's thresholds, as divisors of the node count the schedule refers to (phmrf_solve_state::sched_n)
static const int64_t COARSE_ON_DIV = 8;       // "moved at large": a solve changed >= 1/8 of the labels so far
static const int64_t COARSE_ROUND_DIV = 4;    // "moving at large": a round changed >= 1/4 of the labels (a cold start)
static const int64_t MOVING_DIV_AT_LARGE = 64;   // "this round moved the labelling at large": >= 1/64 of the labels in a solve that has
static const int64_t MOVING_DIV = 16;            //   moved at large in all, >= 1/16 otherwise (fold_counters)
static const int TICK_BUDGET = 60000;         // launch ticks of one solve: the change stamps are 16-bit launch ticks

// The twelve child problems of a block (N_COARSE_CHILDREN: three scales x four labels of a batch) are lean: a child holds what
// coarsen_kernel writes and strip_kernel / coarse_apply_kernel read -- labels, two unary planes, the forward weights, a counter bank -- and
// all twelve come out of ONE device allocation made at the first coarse sweep.  (They used to be full blocks: a stream, three
// pinned host buffers, two events and eleven device buffers each -- some two hundred runtime calls per block, 50 - 60 ms of
// the first cold solve of EVERY block, whatever its size.)
static int coarse_children_create(phmrf_block_t b) {
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  constexpr int NC = N_COARSE_CHILDREN;
  size_t off_lab[NC], off_uT[NC], off_fwd[NC], total = up((size_t)NC * N_COUNTERS * sizeof(unsigned long long));   // the counter banks first
  int64_t nm[NC];
  for (int ls = 0; ls < N_COARSE_CHILDREN; ++ls) {
    const int s = COARSE_SCALE[ls / 4];
    nm[ls] = coarse_nodes(b, s, s - 1);
    off_lab[ls] = total;
    total += up((size_t)nm[ls]);
    off_uT[ls] = total;
    total += up((size_t)2 * nm[ls] * sizeof(float));
    off_fwd[ls] = total;
    total += up((size_t)nm[ls] * sizeof(float4));
  }
  PHMRF_HIP(hipMalloc(reinterpret_cast<void**>(&b->coarse_arena), total));
  PHMRF_HIP(hipMemsetAsync(b->coarse_arena, 0, (size_t)NC * N_COUNTERS * sizeof(unsigned long long), b->stream));
  for (int ls = 0; ls < N_COARSE_CHILDREN; ++ls) {
    phmrf_block* c = new phmrf_block();
    c->n = nm[ls];
    c->S = 1;
    c->K = 2;
    c->device = b->device;
    c->deterministic = b->deterministic;
    c->counters = reinterpret_cast<unsigned long long*>(b->coarse_arena) + (size_t)ls * N_COUNTERS;
    c->labels = reinterpret_cast<uint8_t*>(b->coarse_arena + off_lab[ls]);
    c->uT = reinterpret_cast<float*>(b->coarse_arena + off_uT[ls]);
    c->fwd_w = reinterpret_cast<float4*>(b->coarse_arena + off_fwd[ls]);
    c->uT_valid = true;
    c->has_grid = true;
    c->has_graph = true;
    c->has_logprob = true;
    c->D = 0;
    c->unary_pins = true;
    c->stream = b->stream;
    b->coarse[ls] = c;
  }
  return PHMRF_OK;
}

void coarse_children_destroy(phmrf_block* b) {
  for (int ls = 0; ls < N_COARSE_CHILDREN; ++ls) {
    delete b->coarse[ls];             // (a child owns nothing: its buffers are slices of the arena)
    b->coarse[ls] = nullptr;
  }
  if (b->coarse_arena) (void)hipFree(b->coarse_arena);
  b->coarse_arena = nullptr;
}

int coarse_child(phmrf_block* b, int level_slot, phmrf_block** out) {
  if (!b->coarse_arena) PHMRF_TRY(coarse_children_create(b));
  b->coarse[level_slot]->stream = b->stream;
  b->coarse[level_slot]->num_neighbor = b->num_neighbor;
  *out = b->coarse[level_slot];
  return PHMRF_OK;
}

// every label alpha of `labels_mask` once at one scale / offset: coarsen -> one strip pass per orientation on the
// super-cell grid -> apply.  4 launches per label.
int coarse_sweep_nocount(phmrf_block* b, float beta, int level, int off, int shift_r, int shift_c, int alpha_lo, int alpha_hi,
                         unsigned long long label_mask) {
  const int s = COARSE_SCALE[level];
  if (!b->uT_valid) PHMRF_TRY(launch_unary_planes(b));
  // Labels in batches of four: one pass over the block builds the four child problems (the label-independent two thirds of
  // coarsen_kernel's reads once instead of four times), then label by label the child's two strip passes and the apply
  // pass, in order.  A label whose predecessors in the batch moved something gets its problem rebuilt first -- decided on
  // the device (coarse_apply_kernel raises b->coarse_flag, the one-label rebuild returns at once while it is down): the
  // sequence of labellings is the one-label-at-a-time sequence, the host never waits.  PHMRF_COARSE_BATCH=1: one by one.
  static const int batch_env = PHMRF_DEV_ENV("PHMRF_COARSE_BATCH") ? atoi(PHMRF_DEV_ENV("PHMRF_COARSE_BATCH")) : 4;
  const int batch = (batch_env == 1 || batch_env == 2) ? batch_env : 4;
  static const bool no_gate = PHMRF_DEV_ENV("PHMRF_COARSE_NO_GATE") != nullptr;      // development: A/B timing
  static const bool no_stamp_gate = PHMRF_DEV_ENV("PHMRF_COARSE_NO_STAMP_GATE") != nullptr;
  phmrf_block* ch[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int q = 0; q < batch; ++q) PHMRF_TRY(coarse_child(b, level * 4 + q, &ch[q]));
  if (!b->coarse_flag) PHMRF_TRY(dev_alloc(&b->coarse_flag, (size_t)1));
  tic(b, KC_COARSE);
  int n_launch = 0;
  // (the labels of [alpha_lo, alpha_hi) that `label_mask` lists, ascending, in batches)
  std::vector<int> todo;
  for (int a = alpha_lo; a < alpha_hi; ++a)
    if ((label_mask >> a) & 1ull) todo.push_back(a);
  for (size_t t0 = 0; t0 < todo.size(); t0 += (size_t)batch) {
    const int nl = (int)std::min<size_t>((size_t)batch, todo.size() - t0);
    int alphas[4] = {0, 0, 0, 0};
    for (int q = 0; q < nl; ++q) alphas[q] = todo[t0 + q];
    // The apply pass (a thread per fine node) returns at once when the child's two passes switched no super-cell: the
    // child counts its switches in its own bank (COARSE_CHILD_SLOT), and the apply kernel reads it on the device.  (The batch's pass
    // zeroes those counters and the block's moved-flag itself.)
    for (int q = 0; q < nl; ++q) ch[q]->counter_slot = COARSE_CHILD_SLOT;
    PHMRF_TRY(launch_coarsen_batch(b, ch, alphas, nl == 3 ? 3 : nl, s, off, beta, nullptr, -1, true));
    // (inside a solve the change stamps say WHERE the labels before a label in the batch have moved: its rebuild touches
    //  those wavefronts only -- every apply pass below stamps with a tick later than this one)
    const int since = (b->tick && !no_stamp_gate) ? b->tick : -1;
    ++n_launch;
    for (int q = 0; q < nl; ++q) {
      phmrf_block* c = ch[q];
      if (q > 0) {        // rebuilt only if a label before it in the batch has moved (b->coarse_flag, read on the device)
        phmrf_block* one[1] = {c};
        PHMRF_TRY(launch_coarsen_batch(b, one, &alphas[q], 1, s, off, beta, b->coarse_flag, since, false));
        ++n_launch;
      }
      // (measured: the filtered multi-label kernel is 15-20 % slower than the plain one on these one-label problems)
      PHMRF_TRY(launch_strip_pass(c, beta, 0, shift_r % 6, shift_c % 64, 1, -1));
      PHMRF_TRY(launch_strip_pass(c, beta, 1, (shift_r + 3) % 6, (shift_c + 31) % 64, 1, -1));
      if (b->tick) ++b->tick;
      PHMRF_TRY(launch_coarse_apply(b, c, s, off, alphas[q], no_gate ? nullptr : c->counters + COARSE_CHILD_SLOT, b->coarse_flag,
                                    b->coarse_lab ? b->coarse_lab + level * MAX_LABELS + alphas[q] : nullptr));
      n_launch += 3;
    }
  }
  toc(b, KC_COARSE, n_launch);
  return PHMRF_OK;
}

// The energy after a round of a solve, in two halves: energy_round_launch queues the evaluation behind the round's moves,
// energy_round_collect reads it once the stream has been synchronised.  The first evaluation of a solve is the full pass;
// later ones on a large grid block add the change since the previous evaluation, taken from the nodes the round's moves have
// stamped (energy_delta_grid_kernel) -- a mop-up round touches a few per cent of the block.  Each evaluation leaves a
// snapshot of the labels and its tick behind for the next.  A row tile counts the rows it owns in both passes; the halo
// labels it receives between two evaluations (tile.hip, put_labels_kernel) leave the snapshot alone, so the next
// incremental pass sees them as a change of the tile's edges into its lower halo row.  (Development library:
// PHMRF_ENERGY_FULL=1: always the full pass; PHMRF_ENERGY_CHECK=1: both, compared, tiles included; PHMRF_ENERGY_MIN_N: the
// size from which the incremental pass is taken.)  The carried values are (unary, pair without beta).
static int energy_round_launch(phmrf_block* b, bool* incremental_out, bool* snapshot_out) {
  static const bool always_full = PHMRF_DEV_ENV("PHMRF_ENERGY_FULL") != nullptr;
  // (PHMRF_ENERGY_MIN_N, development library: the size from which the incremental pass is taken, for tests at small shapes)
  static const char* const min_n_env = PHMRF_DEV_ENV("PHMRF_ENERGY_MIN_N");
  static const int64_t min_n = min_n_env ? std::max<int64_t>(1, std::atoll(min_n_env)) : (int64_t)1 << 18;
  const bool grid = b->has_grid && b->fwd_w && b->uT && b->uT_valid && b->stamp && b->tick > 0 && b->n >= min_n;
  const bool snapshot = grid && !always_full;
  const bool incremental = snapshot && energy_delta_available(b);
  // (round 6) the round's two energy sums live in the counter bank (COUNTER_ENERGY: two slots, as doubles -- or 2^-20 fixed-point integers
  // in deterministic mode): the memset that opens the round has zeroed them and the ONE read-back of the bank that closes it
  // carries them -- two fills / copies per round fewer than with the accumulator area
  tic(b, KC_ENERGY);
  double* const at = reinterpret_cast<double*>(b->counters + COUNTER_ENERGY);
  if (incremental) {
    PHMRF_TRY(launch_energy_delta(b, at));
    b->work[WORK_INCREMENTAL] += 1;
  } else {
    PHMRF_TRY(launch_energy(b, 0.f, at));
  }
  toc(b, KC_ENERGY, 1);
  if (is_tile(b))        // (the pin-violation count of a row tile: accum slot 6, tile.hip)
    PHMRF_HIP(hipMemcpyAsync(b->accum_host + 6, b->accum + 6, sizeof(double), hipMemcpyDeviceToHost, b->stream));
  if (snapshot) {       // the snapshot for the next evaluation: every launch from here on carries a later tick
    if (!b->labels_eval) PHMRF_TRY(dev_alloc(&b->labels_eval, (size_t)b->n));
    PHMRF_HIP(hipMemcpyAsync(b->labels_eval, b->labels, (size_t)b->n, hipMemcpyDeviceToDevice, b->stream));
    b->eval_tick = b->tick;
    ++b->tick;
  }
  *incremental_out = incremental;
  *snapshot_out = snapshot;
  return PHMRF_OK;
}

// (the stream has been synchronised)  -> *eu, *ep_raw: unary and pair sum (without beta) after the round
static int energy_round_collect(phmrf_block* b, double beta, bool incremental, double* eu_carry, double* ep_carry) {
  static const bool check = PHMRF_DEV_ENV("PHMRF_ENERGY_CHECK") != nullptr;
  double du, dp;
  energy_sums(b, b->counters_host + COUNTER_ENERGY, &du, &dp);
  if (incremental) {
    *eu_carry += du;
    *ep_carry += dp;
  } else {
    *eu_carry = du;
    *ep_carry = dp;
  }
  if (check && incremental) {
    double fu, fp;
    PHMRF_TRY(energy_now(b, beta, &fu, &fp));
    const double eu = *eu_carry, ep = beta * *ep_carry;
    const double tol = 1e-9 * std::fabs(fu + fp) + 1e-3;
    if (std::fabs(fu - eu) > tol || std::fabs(fp - ep) > tol)
      fprintf(stderr, "[phmrf energy check] incremental %.6f + %.6f, full %.6f + %.6f (diff %.3e, %.3e)\n", eu, ep, fu, fp,
              eu - fu, ep - fp);
  }
  return PHMRF_OK;
}

// ---- the label solver as a resumable state machine ------------------------------------------------------------------
// phmrf_mrf_solve = begin; { round_launch; round_collect; round_decide } until decided; end.  The pieces are entry points
// of their own so that the tiles of ONE block that live on different GPUs can run their rounds in lockstep: between
// collect and decide the host adds up the tiles' change counters and energies (one small all-gather per round), every tile
// takes the same decision from the sums, and the boundary label rows are exchanged (phylo_hmrf_amd/tiles.py).
void solve_scope_exit(phmrf_block* b) {
  phmrf_solve_state* s = b->ss;
  if (s) b->geom_phase = (s->geom + 1) % 3;
  b->tick = 0;
  b->eval_tick = -1;
  b->counter_slot = COUNTER_DEFAULT;
  b->prop_tick = -1;
  delete s;
  b->ss = nullptr;
}

// queue the copy of a tile's first and last owned rows into the pinned staging buffer (top row first); whoever
// synchronises the stream next finds them there (phmrf_block_tile_get_boundary then copies without touching the device)
int tile_queue_boundary(phmrf_block* b) {
  int64_t off = 0;
  if (b->tile_top) {
    const int64_t tf = row_first(b, 1), tc = row_first(b, 2) - tf;
    PHMRF_HIP(hipMemcpyAsync(b->xfer_host, b->labels + tf, (size_t)tc, hipMemcpyDeviceToHost, b->stream));
    off = tc;
  }
  if (b->tile_bot) {
    const int64_t bf = row_first(b, b->H - 2), bc = row_first(b, b->H - 1) - bf;
    PHMRF_HIP(hipMemcpyAsync(b->xfer_host + off, b->labels + bf, (size_t)bc, hipMemcpyDeviceToHost, b->stream));
  }
  b->boundary_queued = true;
  return PHMRF_OK;
}

}  // namespace phmrf

using namespace phmrf;

// A failure inside solve_begin or a solve loop still ends the solves that have begun (those phmrf_mrf_solve_end has not ended) --
// each once nothing of it is queued any more: a round in flight (kernels, read-backs into the pinned buffers) drains first.
struct EndSolves {
  phmrf_block_t* bl;
  int n;
  ~EndSolves() {
    for (int i = 0; i < n; ++i)
      if (bl[i]->ss) {
        (void)hipStreamSynchronize(bl[i]->stream);
        solve_scope_exit(bl[i]);
      }
  }
};

namespace phmrf {
// (the blocks that start coarse-to-fine: a complete 8-neighbour grid that is no row tile and large enough for a coarse grid)
bool c2f_applies(const phmrf_block* b) {
  if (!b->has_grid || !b->fwd_w || b->num_neighbor != 8 || !b->grid_complete || is_tile(b)) return false;
  return b->n >= 1024 && b->H >= 2 * C2F_SCALE && b->W >= 2 * C2F_SCALE;
}

// the child block of the coarse-to-fine start, b->c2f, with its graph and grid tables: built at the first call
int c2f_child(phmrf_block* b) {
  const int s = C2F_SCALE;
  if (!b->c2f) {
    const int Hc = (b->H + s - 1) / s, Wc = (b->W + s - 1) / s;
    Geometry gc(Hc, Wc, b->diagonal);
    phmrf_block_t c = nullptr;
    PHMRF_TRY(phmrf_block_create(gc.count(), 1, b->K, &c));
    // the child becomes b->c2f only once it is complete: a failure on the way destroys it, and the next cold solve starts over
    // (a half-built child -- no graph, no grid tables -- must never be solved on)
    auto build = [&]() -> int {
      c->stream = b->stream;                    // (the child's kernels read the parent's logprob and write its labels)
      PHMRF_TRY(dev_alloc(&c->nbr, (size_t)c->n * 8));
      PHMRF_TRY(dev_alloc(&c->wgt, (size_t)c->n * 8));
      c->D = 8;
      PHMRF_TRY(launch_c2f_graph(b, c, Hc, Wc, s));
      if (!c->colour_nodes) PHMRF_TRY(dev_alloc(&c->colour_nodes, (size_t)c->n));
      c->has_graph = true;
      PHMRF_TRY(setup_grid_tables(c, gc, 8));
      c->grid_complete = true;
      return PHMRF_OK;
    };
    const int st = build();
    if (st != PHMRF_OK) {
      (void)hipStreamSynchronize(b->stream);    // (its kernels were queued on the parent's stream)
      c->stream = c->own_stream;
      (void)phmrf_block_destroy(c);
      return st;
    }
    b->c2f = c;
    b->c2f_Hc = Hc;
    b->c2f_Wc = Wc;
  }
  b->c2f->stream = b->stream;
  return PHMRF_OK;
}
}  // namespace phmrf

// The coarse-to-fine start of a cold solve (c2f.hip): the labelling problem of the block's 4 x 4 super-cells as a block of
// its own (created at the first cold solve; its graph is built once, the graph of the block being constant over a fit),
// solved from ITS cold start by this same solver -- which recurses while the coarse block is large --, and copied down.
// *started: the block's labels are the prolongated coarse labels (otherwise the caller takes argmax_k logprob).
static int c2f_start(phmrf_block* b, double beta, const phmrf_solve_opts& o, bool* started) {
  *started = false;
  if (o.coarse_start <= 0 || !o.use_strips || !c2f_applies(b)) return PHMRF_OK;
  const int s = C2F_SCALE;
  PHMRF_TRY(c2f_child(b));
  phmrf_block* c = b->c2f;
  PHMRF_TRY(launch_c2f_logprob(b, c, b->c2f_Wc, s));
  c->has_logprob = true;
  c->uT_valid = false;
  phmrf_solve_opts oc = o;
  oc.init_mode = 1;
  PHMRF_TRY(phmrf_mrf_solve(c, beta, &oc, nullptr));
  PHMRF_TRY(launch_c2f_prolong(b, c, b->c2f_Wc, s));
  *started = true;
  return PHMRF_OK;
}

// ---- one round, move type by move type ----------------------------------------------------------------------------------
// the launches that follow add their changes to counters[slot], and the slot's move type has run this round
static void count_into(phmrf_block* b, int slot) {
  b->counter_slot = slot;
  b->ss->ran[slot] = 1;
}
static void activate_all(phmrf_solve_state* s) {
  for (int sl : s->slots) s->active[sl] = 1;
}
static bool out_of_budget(const phmrf_block* b) { return b->ss->rounds >= b->ss->o.max_rounds || b->tick >= TICK_BUDGET; }
// the solve has moved the labelling at large in all (a cold or far-off start, not the warm start of a later EM iteration)
static bool moved_at_large(const phmrf_solve_state* s) { return s->total * COARSE_ON_DIV >= s->sched_n; }
// the previous round moved it at large (a cold start)
static bool last_round_moved_at_large(const phmrf_solve_state* s) { return s->last_changed * COARSE_ROUND_DIV >= s->sched_n; }
// Inside a coarse scale the labels rest like the fine expansions' labels do.  Row tiles keep every label (their schedule
// runs on sums over the tiles; the per-label counts are local), and so does an exact solve.
static bool rests_coarse_labels(const phmrf_block* b) { return !is_tile(b) && b->ss->o.energy_tol_ppb > 0; }
// (a verification round tries every shift of every scale -- as long as the solve has moved the labelling at large or runs
//  to the exact fixed point; the warm start of a later EM iteration under a stopping tolerance, which moves 1-3 % of the
//  labels, would pay several times its own cost for them)
static bool verifies_coarse(const phmrf_solve_state* s) { return s->verifying && (s->o.energy_tol_ppb == 0 || moved_at_large(s)); }
static bool coarse_scale_on(const phmrf_solve_state* s, int lv) {
  return verifies_coarse(s) || s->force_coarse ||
         (s->active[COUNTER_COARSE + lv] && (last_round_moved_at_large(s) || s->coarse_changed[lv] > 0));
}
// does a coarse scale run every label: a verification round, the forced last say, a scale switched on by a round that moved at large
static bool coarse_runs_all_labels(const phmrf_block* b) {
  const phmrf_solve_state* s = b->ss;
  return !rests_coarse_labels(b) || verifies_coarse(s) || s->force_coarse || last_round_moved_at_large(s);
}

static int solve_begin(phmrf_block* b, double beta, const phmrf_solve_opts* opts, bool want_init_energy) {
  PHMRF_TRY(check_solvable(b));
  if (b->ss) solve_scope_exit(b);                 // (an abandoned solve)
  phmrf_solve_state* s = new phmrf_solve_state();
  b->ss = s;
  phmrf_solve_opts& o = s->o;
  std::memset(&o, 0, sizeof(o));
  o.max_rounds = 64;
  o.use_chains = 1;
  o.use_components = 1;
  o.use_strips = 1;
  o.use_expansion = 1;
  o.use_coarse = 1;
  if (opts) {
    o = *opts;
    if (o.max_rounds <= 0) o.max_rounds = 64;
  }
  s->beta = beta;
  s->bf = (float)beta;
  s->sched_n = b->sched_n > 0 ? b->sched_n : b->n;
  b->labels_are_slot = 0;                        // (whatever the solve does to the labels)
  EndSolves abort_guard{&b, 1};                   // a failure below leaves no half-begun solve behind
  if (o.init_mode == 1) {
    bool started = false;
    PHMRF_TRY(c2f_start(b, beta, o, &started));        // coarse-to-fine (c2f.hip), where the block qualifies
    if (!started) PHMRF_TRY(launch_argmax_labels(b));
    b->has_labels = true;
  }
  if (want_init_energy) {
    PHMRF_TRY(energy_now(b, beta, &s->eu0, &s->ep0));
    s->have_init_energy = true;
  }
  // a graph without grid geometry gets its path families at its first solve (setup_path_families: once per graph)
  if (o.use_chains && !b->has_grid && b->families.empty() && b->nbr && b->n >= 2) PHMRF_TRY(setup_path_families(b));
  s->chains = o.use_chains && (b->has_grid || !b->families.empty());
  s->strips = o.use_strips && b->has_grid;
  s->tol = o.min_changed > 0 ? o.min_changed : 0;
  const int K = b->K;
  // move types and their change counters (the slots of b->counters, common.h)
  s->expansions = s->strips && o.use_expansion;
  // a graph without grid geometry: every label's alpha-expansion over the WHOLE graph by a minimum cut (maxflow.hip), the
  // move gco's expansion() makes; the same change counters
  s->graph_expansions = !b->has_grid && o.use_expansion && b->nbr != nullptr && b->n >= 2;
  s->n_fam = s->chains ? (int)b->families.size() : 0;
  PHMRF_CHECK(s->n_fam <= MAX_CHAIN_FAMILIES, PHMRF_ERR_INVALID, "internal: more chain families than counter slots");
  for (int f = 0; f < s->n_fam; ++f) s->slots.push_back(COUNTER_CHAIN + f);
  s->slots.push_back(COUNTER_ICM);
  if (o.use_components) s->slots.push_back(COUNTER_COMPONENT);
  if (s->strips) {
    s->slots.push_back(COUNTER_FUSION);
    s->slots.push_back(COUNTER_FUSION + 1);
  }
  if (s->expansions || s->graph_expansions)
    for (int a = 0; a < K; ++a) s->slots.push_back(COUNTER_EXPANSION + a);
  // coarse alpha-expansions: a slot per scale (2 x 2 super-cells, 4 x 4, 8 x 8)
  s->coarse = s->strips && o.use_coarse && b->H >= 4 && b->W >= 4;
  if (s->coarse)
    for (int lv = 0; lv < N_COARSE; ++lv) s->slots.push_back(COUNTER_COARSE + lv);
  activate_all(s);
  s->last_count.fill(-1);
  // change stamps + per-strip memo of quiet expansions (exact skip of strips whose inputs did not change)
  if (!b->stamp) PHMRF_TRY(dev_alloc(&b->stamp, (size_t)b->n));
  PHMRF_HIP(hipMemsetAsync(b->stamp, 0, (size_t)b->n * sizeof(uint16_t), b->stream));
  b->tick = 1;
  b->eval_tick = -1;                   // (no energy evaluation in this solve yet: the first one is a full pass)
  b->prop_tick = -1;
  if (s->chains) {                       // segment memos of all families: one buffer, one memset
    size_t total = 0;
    for (auto& f : b->families)
      for (int p = 0; p < 2; ++p)
        for (int c = 0; c < f.n_colours; ++c) total += (size_t)f.nseg[p][c];
    if (!b->chain_memo || b->chain_memo_count != total) {
      dev_free(b->chain_memo);
      PHMRF_TRY(dev_alloc(&b->chain_memo, total));
      b->chain_memo_count = total;
    }
    size_t off = 0;
    for (auto& f : b->families)
      for (int p = 0; p < 2; ++p)
        for (int c = 0; c < f.n_colours; ++c) {
          f.memo[p][c] = f.nseg[p][c] > 0 ? b->chain_memo + off : nullptr;
          off += (size_t)f.nseg[p][c];
        }
    PHMRF_HIP(hipMemsetAsync(b->chain_memo, 0, (total ? total : 1) * sizeof(uint16_t), b->stream));
  }
  if (s->strips) {                         // (the fusion passes keep a memo, too: slot K)
    int64_t max_strips = 0;
    for (int orient = 0; orient < 2; ++orient) {
      const int Hs = orient ? b->W : b->H, Ws = orient ? b->H : b->W;
      const int64_t ns = (int64_t)((Hs + 5 + 5) / 6) * ((Ws + 63 + 63) / 64);
      max_strips = std::max(max_strips, ns);
    }
    if (!b->memo || b->memo_strips < max_strips) {
      dev_free(b->memo);
      PHMRF_TRY(dev_alloc(&b->memo, (size_t)6 * max_strips * (K + 1)));
      b->memo_strips = max_strips;
    }
    PHMRF_HIP(hipMemsetAsync(b->memo, 0, (size_t)6 * b->memo_strips * (K + 1) * sizeof(uint16_t), b->stream));
  }
  // One round runs every ACTIVE move type: chain families, ICM, component moves, strip fusion per orientation, strip
  // alpha-expansion per label.  A type stays active while it still changes labels.  When a round is quiet (at most
  // `min_changed` labels changed, or the energy did not go down) a VERIFICATION round with every type active (and the
  // chain segments cut at their other set of separators) decides: quiet again -> done.  (The energy test also ends the
  // alternation between two labellings of exactly equal energy that different move types prefer; gco stops on the same
  // criterion, GCoptimization.cpp:1298.)
  // the energy before the first round (only needed when the caller asked for it: the first round of a solve that
  // changes labels always improves, and the tolerance refers to the energy after the round).  The tiles of a split block
  // start without it: their schedule runs on sums over the tiles, which begin with the first round's.
  s->e_prev = (s->have_init_energy && !is_tile(b)) ? s->eu0 + s->ep0 : std::numeric_limits<double>::infinity();
  // The strip alpha-expansions run on one of three fixed cuts (so that the per-strip memo of quiet runs applies).  The
  // cut ADVANCES after a round that moved the labelling at large (>= 1/64 of the labels: the memo is worth little
  // then), when a verification round begins, and from one solve to the next (b->geom_phase); it STAYS while the solve
  // is mopping up, so those rounds only revisit the strips whose inputs changed -- a warm start pays for one full
  // sweep per solve instead of one per round.
  s->geom = b->geom_phase % 3;
  if (is_tile(b)) PHMRF_TRY(zero_accum(b, 6, 1));       // the pin-violation counter (tile.hip)
  abort_guard.n = 0;
  return PHMRF_OK;
}

// Chain moves (exact 1-D Viterbi over all K labels): with the strip expansions in place they run in verification
// rounds only.  Measured (round 2, live-gco parity cases and the whole-genome bench): in ordinary rounds they make
// 60 % of a warm start's label changes but the strips find the same energy without them -- the 2,001,000-node
// K=10 cold start even ends 2e-4 LOWER and in 12 rounds instead of 32 (1-D moves leave row / column streaks that
// the 2-D moves then have to undo) -- and they were 14 % of the device time.  Without strip expansions (general
// graphs have no chains at all; `use_expansion = 0`) rows and columns run in every round as before.
static int round_chains(phmrf_block* b) {
  phmrf_solve_state* s = b->ss;
  const int n_ord_fams = s->expansions ? 0 : (b->has_grid ? 2 : s->n_fam);     // (path families of a general graph: all of them)
  auto runs = [&](int f) { return s->active[COUNTER_CHAIN + f] && (f < n_ord_fams || s->verifying); };
  int n_chain = 0;
  for (int f = 0; f < s->n_fam; ++f)
    if (runs(f)) n_chain += b->families[f].n_colours;
  if (n_chain == 0) return PHMRF_OK;
  tic(b, KC_CHAIN);
  for (int f = 0; f < s->n_fam; ++f)
    if (runs(f)) {
      count_into(b, COUNTER_CHAIN + f);
      // cut phase 0 in ordinary rounds (so the segment memo applies from the second round on); the other set of
      // separators is used by the verification rounds
      // (the path families of a general graph hold two independent decompositions as their two phases: they take
      //  turns round by round, so the round that verifies a quiet one always looks along the other set of paths)
      PHMRF_TRY(chain_sweep_nocount(b, s->bf, f, b->has_grid ? (s->verifying ? 1 : 0) : (s->rounds & 1), false));
    }
  toc(b, KC_CHAIN, n_chain);
  return PHMRF_OK;
}

// single-site ICM: every strip cell and every chain node is already optimal given the rest, so ICM only earns its
// launches on the fixed separator cells; it runs in verification rounds and on graphs without grid moves
static int round_icm(phmrf_block* b) {
  phmrf_solve_state* s = b->ss;
  if (!(s->active[COUNTER_ICM] && (s->verifying || !(s->chains || s->strips) || !b->has_grid))) return PHMRF_OK;
  count_into(b, COUNTER_ICM);
  return icm_sweep_nocount(b, s->bf);
}

// component moves: a full pass over the block (seven kernels) whatever the number of labels that changed.  On grid
// blocks they run in a solve's first round, after a round that moved the labelling at large, and in verification
// rounds; the mop-up rounds in between (a few hundred changed labels, of which the pass would take a dozen) skip
// them.  On general graphs, where they are one of two move types, they run in every round.
static int round_components(phmrf_block* b) {
  phmrf_solve_state* s = b->ss;
  const bool comp_round = s->rounds == 0 || s->verifying || s->prev_moving || !(s->chains || s->strips) || !b->has_grid;
  // (after a round that moved the labelling at large the pass runs whether or not it was rested: its last count is old)
  if (!(s->o.use_components && (s->active[COUNTER_COMPONENT] || s->prev_moving) && comp_round)) return PHMRF_OK;
  count_into(b, COUNTER_COMPONENT);
  if (b->tick) ++b->tick;
  tic(b, KC_COMPONENT);
  PHMRF_TRY(launch_component_pass(b, s->bf));
  toc(b, KC_COMPONENT, 1);
  return PHMRF_OK;
}

// a graph without grid geometry: every active label's alpha-expansion over the whole graph (maxflow.hip)
// (host-synchronous launches: a few small read-backs per expansion; general graphs are off the hot path)
static int round_graph_expansions(phmrf_block* b) {
  phmrf_solve_state* s = b->ss;
  if (!s->graph_expansions) return PHMRF_OK;
  for (int a = 0; a < b->K; ++a)
    if (s->active[COUNTER_EXPANSION + a]) {
      count_into(b, COUNTER_EXPANSION + a);
      ++b->tick;
      tic(b, KC_STRIP);
      PHMRF_TRY(launch_graph_expansion(b, s->bf, a));
      toc(b, KC_STRIP, 1);
    }
  return PHMRF_OK;
}

// per orientation: the strip fusion pass, then every active label's strip expansion
static int round_strips(phmrf_block* b) {
  phmrf_solve_state* s = b->ss;
  if (!s->strips) return PHMRF_OK;
  const int K = b->K, geom = s->geom;
  for (int orient = 0; orient < 2; ++orient) {
    if (s->active[COUNTER_FUSION + orient]) {
      count_into(b, COUNTER_FUSION + orient);
      // the fusion pass runs on a cut of its own that moves with the expansions' (so that its memo of quiet strips
      // applies while the cut stays): the expansion cut shifted by half a band / half a segment
      PHMRF_TRY(strip_pass_nocount(b, s->bf, orient, (GEOM_R[geom] + 3) % 6, (GEOM_C[geom] + 31) % 64, -1, geom));
    }
    if (!s->expansions) continue;
    // every active label's expansion of the cut in ONE launch: a wave owns a strip, stages it once and runs the
    // labels back to back behind the exact filter (strip_cols_kernel, which counts label a into COUNTER_EXPANSION + a itself)
    unsigned long long lmask = 0ull;
    for (int a = 0; a < K; ++a)
      if (s->active[COUNTER_EXPANSION + a]) {
        lmask |= 1ull << a;
        s->ran[COUNTER_EXPANSION + a] = 1;
      }
    if (!lmask) continue;
    if (!b->uT_valid) {
      tic(b, KC_PROPOSE);
      PHMRF_TRY(launch_unary_planes(b));
      toc(b, KC_PROPOSE, 1);
    }
    tic(b, KC_STRIP);
    ++b->tick;
    PHMRF_TRY(launch_strip_multi(b, s->bf, orient, GEOM_R[geom], GEOM_C[geom], lmask, geom));
    b->tick += K;                           // one tick per label inside the launch
    b->work[4] += 1;
    toc(b, KC_STRIP, 1);
  }
  return PHMRF_OK;
}

// coarse alpha-expansions.  Coarse scales switch on while the labelling is still moving at large (the previous round
// changed >= 25 % of the labels: a cold start).  A solve that has moved >= 12.5 % of the labels in all (a far-off warm
// start of an EM iteration) gets them once at the end, before the tolerance may stop it (force_coarse below); the warm
// start of a later EM iteration, which moves 1-3 %, does not pay for them at all.
// A scale that changed labels in its last run stays on (like every move type), with the super-cell grid shifted by
// one node per round; a verification round tries every shift of both scales.
// Round 5: inside a scale the LABELS rest like the fine expansions' labels do: a label whose expansion at this scale
// changed nothing in its last run is left out until the scale is switched on afresh (a round that moved the labelling at
// large), a verification round or the forced last say runs all labels again.  A coarse round costs what its labels cost
// -- a share of the coarsen pass, two child strip passes and an apply pass each --, and after the first coarse round of a
// cold or far-off solve a few labels per scale are still moving (measured: HISTORY.md 3.1 item 6, round 5).
static int round_coarse(phmrf_block* b) {
  phmrf_solve_state* s = b->ss;
  if (!s->coarse) return PHMRF_OK;
  const int K = b->K, r = s->rounds;
  const size_t lab_bytes = (size_t)N_COARSE * MAX_LABELS * sizeof(unsigned long long);
  bool any_on = false;
  for (int lv = 0; lv < N_COARSE; ++lv) any_on = any_on || coarse_scale_on(s, lv);
  const bool count_labels = any_on && rests_coarse_labels(b);     // labels changed per scale and label -> b->coarse_lab
  if (count_labels) {
    if (!b->coarse_lab) {
      PHMRF_TRY(dev_alloc(&b->coarse_lab, (size_t)N_COARSE * MAX_LABELS));
      PHMRF_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->coarse_lab_host), lab_bytes));
    }
    PHMRF_HIP(hipMemsetAsync(b->coarse_lab, 0, lab_bytes, b->stream));
  }
  const bool verify_coarse = verifies_coarse(s), all_labels = coarse_runs_all_labels(b);
  const unsigned long long kmask = K >= MAX_LABELS ? ~0ull : ((1ull << K) - 1ull);
  for (int lv = 0; lv < N_COARSE; ++lv) {
    const int sc = COARSE_SCALE[lv];
    s->coarse_ran[lv] = coarse_scale_on(s, lv);
    if (!s->coarse_ran[lv]) continue;
    if (all_labels) s->coarse_lab_mask[lv] = kmask;
    s->coarse_all[lv] = all_labels;
    count_into(b, COUNTER_COARSE + lv);
    for (int off = 0; off < sc; ++off)
      if (verify_coarse || off == r % sc)
        PHMRF_TRY(coarse_sweep_nocount(b, s->bf, lv, off, (2 * r + lv + off) % 6, (17 * r + 5 * lv + 13 * off) % 64, 0, K,
                                       s->coarse_lab_mask[lv] & kmask));
  }
  if (count_labels)
    PHMRF_HIP(hipMemcpyAsync(b->coarse_lab_host, b->coarse_lab, lab_bytes, hipMemcpyDeviceToHost, b->stream));
  return PHMRF_OK;
}

// queue one round: every active move type, then the energy evaluation and the read-back of the change counters
int phmrf_mrf_solve_round_launch(phmrf_block_t b) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  phmrf_solve_state* s = b->ss;
  PHMRF_CHECK(s, PHMRF_ERR_STATE, "no solve in progress (phmrf_mrf_solve_begin)");
  PHMRF_CHECK(!s->launched, PHMRF_ERR_STATE, "the previous round has not been decided");
  if (s->status != 0) return PHMRF_OK;
  PHMRF_HIP(hipMemsetAsync(b->counters, 0, N_COUNTERS * sizeof(unsigned long long), b->stream));
  s->ran.fill(0);
  PHMRF_TRY(round_chains(b));
  PHMRF_TRY(round_icm(b));
  PHMRF_TRY(round_components(b));
  PHMRF_TRY(round_graph_expansions(b));
  PHMRF_TRY(round_strips(b));
  PHMRF_TRY(round_coarse(b));
  b->counter_slot = COUNTER_DEFAULT;
  if (b->timing) PHMRF_TRY(work_fetch_async(b));
  PHMRF_TRY(energy_round_launch(b, &s->incremental, &s->snapshot));
  PHMRF_HIP(hipMemcpyAsync(b->counters_host, b->counters, N_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           b->stream));       // (the change counters AND the round's energy sums, COUNTER_ENERGY)
  if (is_tile(b)) PHMRF_TRY(tile_queue_boundary(b));      // the rows the neighbours need travel with the counters
  s->launched = true;
  s->collected = false;
  return PHMRF_OK;
}

// wait for the round; -> this block's change counters [N_COUNTERS] and its (unary, pair without beta) energy after the round
int phmrf_mrf_solve_round_collect(phmrf_block_t b, uint64_t* counters, double* energy) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  phmrf_solve_state* s = b->ss;
  PHMRF_CHECK(s, PHMRF_ERR_STATE, "no solve in progress (phmrf_mrf_solve_begin)");
  if (s->status != 0 && !s->launched) {            // decided already: nothing ran
    if (counters) std::memset(counters, 0, N_COUNTERS * sizeof(unsigned long long));
    if (energy) { energy[0] = s->eu_carry; energy[1] = s->ep_carry; }
    return PHMRF_OK;
  }
  PHMRF_CHECK(s->launched, PHMRF_ERR_STATE, "no round has been launched");
  if (!s->collected) {
    PHMRF_HIP(hipStreamSynchronize(b->stream));
    PHMRF_TRY(energy_round_collect(b, s->beta, s->incremental, &s->eu_carry, &s->ep_carry));
    if (b->timing) work_fold(b, s->rounds == 0);
    s->collected = true;
    if (is_tile(b)) {
      unsigned long long viol = 0;
      std::memcpy(&viol, b->accum_host + 6, sizeof(viol));
      PHMRF_CHECK(viol == 0, PHMRF_ERR_STATE, "internal: a pinned row of a tile has moved");
    }
  }
  if (counters) {
    std::memcpy(counters, b->counters_host, N_COUNTERS * sizeof(unsigned long long));
    counters[COUNTER_ENERGY] = counters[COUNTER_ENERGY + 1] = 0ull;     // (the energy sums travel in `energy`, not as counters)
  }
  if (energy) { energy[0] = s->eu_carry; energy[1] = s->ep_carry; }
  return PHMRF_OK;
}

// ---- the schedule: what a round's change counters and energy mean for the next round ------------------------------------
static int finish(phmrf_solve_state* s, int st, int* status) {       // st 1: converged
  s->status = st;
  s->converged = st == 1;
  if (status) *status = st;
  return PHMRF_OK;
}
static int next_round(phmrf_block* b, int* status) {
  if (out_of_budget(b)) return finish(b->ss, 2, status);
  if (status) *status = 0;
  return PHMRF_OK;
}

// the round's counters into the solve's state; -> the labels the round changed
static int64_t fold_counters(phmrf_block* b, const uint64_t* counters) {
  phmrf_solve_state* s = b->ss;
  int64_t ch = 0;
  for (int sl : s->slots) {
    ch += (int64_t)counters[sl];
    if (s->ran[sl]) s->last_count[sl] = (long long)counters[sl];
  }
  s->total += ch;
  s->last_changed = ch;
  // "this round moved the labelling at large" (the cut advances, the component pass runs again): >= 1/64 of the labels
  // in a solve that has moved at large in all (a cold or far-off start: every new cut finds more), >= 1/16 otherwise --
  // the first round of a warm-started E-step moves 1-3 %, and with the rule at 1/64 its second round was a full sweep on
  // a new cut plus a component pass: 162 instead of 121 ms per E-step on the whole-genome workload for 1e-6 of energy
  s->prev_moving = ch * (moved_at_large(s) ? MOVING_DIV_AT_LARGE : MOVING_DIV) >= s->sched_n;
  if (s->prev_moving) s->geom = (s->geom + 1) % 3;
  for (int lv = 0; lv < N_COARSE; ++lv)
    if (s->coarse_ran[lv]) {
      s->coarse_changed[lv] = (int64_t)counters[COUNTER_COARSE + lv];
      // the labels that moved something at this scale stay; the others rest (round_coarse decides when all run again)
      if (b->coarse_lab_host && rests_coarse_labels(b)) {
        unsigned long long keep = 0ull;
        for (int a = 0; a < b->K; ++a)
          if (b->coarse_lab_host[lv * MAX_LABELS + a] > 0ull) keep |= 1ull << a;
        s->coarse_lab_mask[lv] = keep;
      }
    }
  ++s->rounds;
  return ch;
}

// PHMRF_SOLVE_TRACE: one line per round, and with the timers on the round's time per kernel class (development aid, one
// block at a time; tools/cold_trace.py reads the lines)
static void trace_round(phmrf_block* b, const uint64_t* counters, int64_t ch, double e_now) {
  static const bool trace = getenv("PHMRF_SOLVE_TRACE") != nullptr;
  if (!trace) return;
  const phmrf_solve_state* s = b->ss;
  int n_active = 0;
  for (int sl : s->slots) n_active += s->active[sl];
  fprintf(stderr, "[phmrf solve] round %d active %d/%d changed %lld energy %.6f delta %.3e\n", s->rounds - 1, n_active,
          (int)s->slots.size(), (long long)ch, e_now, e_now - s->e_prev);
  if (!b->timing) return;
  static double seen[PHMRF_NUM_KERNEL_CLASSES] = {};      // per-round time of each kernel class (ms)
  resolve_timing(b);
  fprintf(stderr, "[phmrf solve]   ms:");
  static const char* NM[PHMRF_NUM_KERNEL_CLASSES] = {"emis", "icm", "chain", "comp", "energy", "post", "strip", "prop", "coarse", "fusion"};
  for (int kc = 0; kc < PHMRF_NUM_KERNEL_CLASSES; ++kc) {
    fprintf(stderr, " %s %.2f", NM[kc], b->ms[kc] - seen[kc]);
    seen[kc] = b->ms[kc];
  }
  fprintf(stderr, "  changed by slot:");
  for (int sl : s->slots)
    if (counters[sl]) fprintf(stderr, " %d:%llu", sl, (unsigned long long)counters[sl]);
  fprintf(stderr, "\n");
  const unsigned long long* t = b->counters_host + COUNTER_TRACE;
  if (t[TRACE_SEEN])
    fprintf(stderr, "[phmrf solve]   expansion strips: launched %llu, past memo+mask %llu, into DP %llu, DP steps %llu, with a move %llu\n",
            t[TRACE_SEEN], t[TRACE_PAST_MEMO], t[TRACE_INTO_DP], t[TRACE_DP_STEPS], t[TRACE_MOVED]);
}

// accepted tolerance: the round (all active types; the rested ones were worth at most a quarter of the tolerance
// together, see rest_move_types) changed the energy by less than the tolerance.  A round that RAISED the energy by the
// tolerance or more (f32 move arithmetic against the f64 energy) is not "converged": it is quiet, and the
// verification round decides.  -> true: decided (*status is set)
static bool tolerance_decides(phmrf_block* b, double gain, bool coarse_moved, int* status) {
  phmrf_solve_state* s = b->ss;
  const phmrf_solve_opts& o = s->o;
  bool coarse_just_ran = s->coarse;
  for (int lv = 0; lv < N_COARSE; ++lv) coarse_just_ran = coarse_just_ran && s->coarse_ran[lv];
  // (round 5) under a stopping tolerance the coarse scales have their forced "last say" ONCE per solve: it runs every label at
  // every scale, and the rounds after it -- the scales stay on while they move labels, with the labels that moved nothing at
  // rest -- end when a whole round gains less than the tolerance, like any other round.  Until round 5 every coarse move asked
  // for another forced round before the solve might stop (measured on the cold solve of the 12.4 M-node block: two of them, 17
  // of 73 ms, for 1.4 of energy at a tolerance of 59; one more after the rule was tied to the number of labels moved since: 8.5 of
  // 62 ms for 26).  Exact solves (tolerance 0) and row tiles keep the old rule.
  if (coarse_moved && (o.energy_tol_ppb == 0 || is_tile(b))) s->coarse_checked = false;
  s->force_coarse = false;
  // (|gain| below the tolerance on either side: a round that moved three labels and changed the f64 energy sum by
  //  2e-13 of itself, up or down, has converged; a rise of the tolerance's size or more has not -- the verification
  //  round decides then)
  if (!(o.energy_tol_ppb > 0 && std::fabs(gain) < 1e-9 * o.energy_tol_ppb * std::fabs(s->e_prev))) return false;
  // A solve that has moved the labelling at large (>= 12.5 % of the labels so far: a cold or far-off start, not the
  // warm start of a later EM iteration) does not stop before the coarse scales have run once more and gained less
  // than the tolerance, too: their gains come in few large steps, not in the trickle the tolerance watches.
  if (s->coarse && !s->coarse_checked && !coarse_just_ran && moved_at_large(s)) {
    s->coarse_checked = true;
    s->force_coarse = true;
    activate_all(s);
    next_round(b, status);
    return true;
  }
  finish(s, 1, status);
  return true;
}

// A quiet round (at most `min_changed` labels changed, or the energy did not go down) asks for a VERIFICATION round with
// every type active, on the next cut; a quiet verification round ends the solve.  -> true: decided (*status is set)
static bool quiet_decides(phmrf_block* b, int64_t ch, bool improved, int* status) {
  phmrf_solve_state* s = b->ss;
  if (!(ch <= s->tol || !improved)) return false;
  if (s->all_active && s->verifying) {
    finish(s, 1, status);
    return true;
  }
  activate_all(s);
  s->all_active = true;
  s->verifying = true;
  if (!s->prev_moving) s->geom = (s->geom + 1) % 3;
  next_round(b, status);
  return true;
}

// A type stays active while it changes labels.  With an energy tolerance the types whose last run changed the
// fewest labels are rested until the verification round, as long as ALL rested types together were worth at most a
// quarter of the stopping tolerance at this round's average gain per changed label (a heuristic about label counts, not
// a bound on the energy a tolerance stop leaves behind: that is what the parity tests against gco measure).
static void rest_move_types(phmrf_block* b, int64_t ch, double gain, bool coarse_moved) {
  phmrf_solve_state* s = b->ss;
  const phmrf_solve_opts& o = s->o;
  auto& active = s->active;
  activate_all(s);
  if (o.energy_tol_ppb > 0 && ch > 0 && gain > 0) {
    const double budget_labels = 1e-9 * o.energy_tol_ppb * std::fabs(s->e_prev) / 4.0 / (gain / (double)ch);
    // (only types that have run in this solve can be rested, on the count of their last run)
    std::vector<int> by_count;
    for (int sl : s->slots)
      if (s->last_count[sl] >= 0) by_count.push_back(sl);
    std::sort(by_count.begin(), by_count.end(), [&](int a, int c) { return s->last_count[a] < s->last_count[c]; });
    double used = 0.0;
    for (int sl : by_count) {
      used += (double)s->last_count[sl];
      if (used > budget_labels) break;
      active[sl] = 0;
    }
  } else {
    for (int sl : s->slots) active[sl] = s->last_count[sl] != 0 ? 1 : 0;
  }
  // (round 5) labels that a coarse scale has just moved are new inputs for the fine moves around them: the strip fusion and
  // the strip expansions run in the next round even if their own last counts had put them to rest -- their memos of quiet
  // strips keep that to the strips near the coarse changes.  (Before, they waited for the forced round: on the cold solve
  // of the 12.4 M-node block five coarse rounds moved 6,245 labels while the fine moves rested, and the forced round after
  // them then found 680 of energy in the fine moves -- twelve tolerances that every earlier stop would have left behind.)
  if (coarse_moved && s->strips && rests_coarse_labels(b)) {
    active[COUNTER_FUSION] = active[COUNTER_FUSION + 1] = 1;
    if (s->expansions)
      for (int a = 0; a < b->K; ++a) active[COUNTER_EXPANSION + a] = 1;
  }
  int n_act = 0;
  for (int sl : s->slots) n_act += active[sl];
  s->all_active = n_act == (int)s->slots.size();
  if (n_act == 0) {
    activate_all(s);
    s->all_active = true;
  }
}

// the schedule: what the round's change counters and energy (of this block, or the sums over the tiles of a split block)
// mean for the next round.  *status: 0 another round, 1 converged, 2 stopped by max_rounds / the launch budget
int phmrf_mrf_solve_round_decide(phmrf_block_t b, const uint64_t* counters, const double* energy, int* status) {
  PHMRF_CHECK(b && counters && energy, PHMRF_ERR_INVALID, "NULL argument");
  phmrf_solve_state* s = b->ss;
  PHMRF_CHECK(s, PHMRF_ERR_STATE, "no solve in progress (phmrf_mrf_solve_begin)");
  if (s->status != 0) {
    if (status) *status = s->status;
    return PHMRF_OK;
  }
  PHMRF_CHECK(s->launched && s->collected, PHMRF_ERR_STATE, "round_decide needs a launched and collected round");
  s->launched = false;
  const double e_now = energy[0] + s->beta * energy[1];
  const int64_t ch = fold_counters(b, counters);
  const bool improved = std::isinf(s->e_prev) ? ch > 0 : e_now < s->e_prev - 1e-11 * std::fabs(s->e_prev);
  trace_round(b, counters, ch, e_now);
  const double gain = s->e_prev - e_now;
  if (e_now < s->e_prev) s->e_prev = e_now;
  bool coarse_moved = false;
  for (int lv = 0; lv < N_COARSE; ++lv) coarse_moved = coarse_moved || (s->coarse && s->coarse_ran[lv] && s->coarse_changed[lv] > 0);
  if (tolerance_decides(b, gain, coarse_moved, status)) return PHMRF_OK;
  if (quiet_decides(b, ch, improved, status)) return PHMRF_OK;
  s->verifying = false;
  rest_move_types(b, ch, gain, coarse_moved);
  return next_round(b, status);
}

int phmrf_mrf_solve_end(phmrf_block_t b, phmrf_solve_result* res) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  phmrf_solve_state* s = b->ss;
  PHMRF_CHECK(s, PHMRF_ERR_STATE, "no solve in progress (phmrf_mrf_solve_begin)");
  if (s->launched && !s->collected) (void)hipStreamSynchronize(b->stream);
  b->has_labels = true;
  int st = PHMRF_OK;
  if (res) {
    double eu = 0, ep = 0;
    st = energy_now(b, s->beta, &eu, &ep);
    res->energy = eu + ep;
    res->energy_unary = eu;
    res->energy_pair = ep;
    res->energy_init = s->have_init_energy ? s->eu0 + s->ep0 : std::numeric_limits<double>::quiet_NaN();
    res->rounds = s->rounds;
    res->converged = s->converged;
    res->changed = s->total;
  }
  static const bool child_count = PHMRF_DEV_ENV("PHMRF_CHILD_COUNT") != nullptr;     // development (with PHMRF_SOLVE_TRACE)
  if (child_count) {
    (void)hipStreamSynchronize(b->stream);
    for (int lv = 0; lv < N_COARSE; ++lv) {
      unsigned long long tot[N_TRACE] = {};
      for (int q = 0; q < 4; ++q) {
        if (!b->coarse[lv * 4 + q]) continue;
        unsigned long long c[N_TRACE];      // (a child's passes count into the trace counters of the child's own bank)
        if (hipMemcpy(c, b->coarse[lv * 4 + q]->counters + COUNTER_TRACE, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) continue;
        for (int x = 0; x < N_TRACE; ++x) tot[x] += c[x];
      }
      fprintf(stderr, "[phmrf solve] coarse scale %d child strips: seen %llu, past the memo and the pin look %llu, into the DP %llu, DP steps %llu, with a move %llu\n",
              COARSE_SCALE[lv], tot[TRACE_SEEN], tot[TRACE_PAST_MEMO], tot[TRACE_INTO_DP], tot[TRACE_DP_STEPS], tot[TRACE_MOVED]);
    }
  }
  solve_scope_exit(b);
  return st;
}

int phmrf_mrf_solve_begin(phmrf_block_t b, double beta, const phmrf_solve_opts* opts, int want_init_energy) {
  return solve_begin(b, beta, opts, want_init_energy != 0);
}

int phmrf_mrf_solve(phmrf_block_t b, double beta, const phmrf_solve_opts* opts, phmrf_solve_result* res) {
  PHMRF_TRY(solve_begin(b, beta, opts, res != nullptr));
  EndSolves scope{&b, 1};
  int status = 0;
  uint64_t counters[N_COUNTERS];
  double energy[2];
  while (status == 0) {
    if (out_of_budget(b)) break;
    PHMRF_TRY(phmrf_mrf_solve_round_launch(b));
    PHMRF_TRY(phmrf_mrf_solve_round_collect(b, counters, energy));
    PHMRF_TRY(phmrf_mrf_solve_round_decide(b, counters, energy, &status));
  }
  return phmrf_mrf_solve_end(b, res);
}

// Several blocks solved in LOCKSTEP ROUNDS from one host thread (round 6): every undecided block's round is queued on its own
// stream, then the rounds are collected and decided in the same order -- the blocks' kernels overlap on the GPU as they do
// when a host thread per block drives them, without the threads.  Each block's state machine is the one phmrf_mrf_solve
// runs: block for block the same labelling (bit-identical under PHMRF_DETERMINISTIC=1).
int phmrf_mrf_solve_group(phmrf_block_t* blocks, int n_blocks, double beta, const phmrf_solve_opts* opts) {
  PHMRF_CHECK(blocks && n_blocks >= 0, PHMRF_ERR_INVALID, "NULL argument");
  for (int i = 0; i < n_blocks; ++i) PHMRF_CHECK(blocks[i], PHMRF_ERR_INVALID, "block is NULL");
  EndSolves scope{blocks, 0};
  for (int i = 0; i < n_blocks; ++i) {
    PHMRF_TRY(solve_begin(blocks[i], beta, opts, false));
    scope.n = i + 1;
  }
  std::vector<int> status(n_blocks, 0);
  std::vector<char> in_flight(n_blocks, 0);
  uint64_t counters[N_COUNTERS];
  double energy[2];
  // queue a block's next round, unless it is decided or out of rounds
  auto launch = [&](int i) -> int {
    phmrf_block* b = blocks[i];
    if (status[i] != 0) return PHMRF_OK;
    if (out_of_budget(b)) {
      status[i] = 2;
      return PHMRF_OK;
    }
    PHMRF_TRY(phmrf_mrf_solve_round_launch(b));
    in_flight[i] = 1;
    return PHMRF_OK;
  };
  int n_in_flight = 0;
  for (int i = 0; i < n_blocks; ++i) {
    PHMRF_TRY(launch(i));
    n_in_flight += in_flight[i];
  }
  // (round 6) the rounds are taken as they END: this thread looks at the streams in turn (hipStreamQuery), and a block whose
  // round has drained is collected, decided and given its next round at once -- no block waits for another's round.  (The
  // first form queued a round of every block, then collected them all in order: 69 - 71 ms per E-step of the whole-genome
  // workload where fourteen threads take 60 - 63.)
  while (n_in_flight > 0) {
    bool progressed = false;
    for (int i = 0; i < n_blocks; ++i) {
      if (!in_flight[i]) continue;
      const hipError_t q = hipStreamQuery(blocks[i]->stream);
      if (q == hipErrorNotReady) continue;
      PHMRF_HIP(q);
      PHMRF_TRY(phmrf_mrf_solve_round_collect(blocks[i], counters, energy));
      PHMRF_TRY(phmrf_mrf_solve_round_decide(blocks[i], counters, energy, &status[i]));
      in_flight[i] = 0;
      --n_in_flight;
      PHMRF_TRY(launch(i));
      n_in_flight += in_flight[i];
      progressed = true;
    }
    if (!progressed) std::this_thread::yield();
  }
  int st = PHMRF_OK;
  for (int i = 0; i < n_blocks; ++i) {
    const int s1 = phmrf_mrf_solve_end(blocks[i], nullptr);
    if (s1 != PHMRF_OK) st = s1;
  }
  scope.n = 0;
  return st;
}
