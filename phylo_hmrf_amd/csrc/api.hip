// C ABI of libphmrf (include/phmrf.h): host-side orchestration around the gfx950 kernels.

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <thread>

#include "common.h"

namespace phmrf {

static thread_local std::string g_error;

void set_error(const std::string& msg) { g_error = msg; }

int fail(int status, const std::string& msg) {
  g_error = msg;
  return status;
}

static hipEvent_t take_event(phmrf_block* b) {
  if (!b->free_events.empty()) {
    hipEvent_t e = b->free_events.back();
    b->free_events.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;   // the interval is then dropped (tic / toc), never mis-timed
  return e;
}

void tic(phmrf_block* b, int kclass) {
  if (!b->timing || !((b->timing_mask >> kclass) & 1u)) return;
  b->cur_start = take_event(b);
  if (b->cur_start && hipEventRecord(b->cur_start, b->stream) != hipSuccess) {
    b->free_events.push_back(b->cur_start);
    b->cur_start = nullptr;
  }
}

void toc(phmrf_block* b, int kclass, int n_launches) {
  const bool first = b->ss && b->ss->rounds == 0;           // (a launch of the first round of a solve: the full sweeps)
  b->launches[kclass] += n_launches;
  if (first) b->launches_first[kclass] += n_launches;
  if (!b->timing || !b->cur_start) return;
  hipEvent_t e = take_event(b);
  if (e && hipEventRecord(e, b->stream) == hipSuccess) {
    b->pending.push_back({kclass, b->cur_start, e, first});
  } else {                                                  // no event: this interval is not timed
    if (e) b->free_events.push_back(e);
    b->free_events.push_back(b->cur_start);
  }
  b->cur_start = nullptr;
}

// One time base per device for all blocks: intervals of different blocks (streams) can be laid on one time line
// (bench.py merges them: the time during which AT LEAST ONE kernel of a class was running).
static hipEvent_t g_time_base[64] = {};

void resolve_timing(phmrf_block* b) {
  if (b->pending.empty()) return;
  (void)hipStreamSynchronize(b->stream);
  hipEvent_t base = (b->device >= 0 && b->device < 64) ? g_time_base[b->device] : nullptr;
  for (auto& p : b->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      b->ms[p.kclass] += ms;
      if (p.first) b->ms_first[p.kclass] += ms;
      float t0 = 0.f;
      if (base && hipEventElapsedTime(&t0, base, p.a) == hipSuccess) b->intervals.push_back({p.kclass, t0, t0 + ms});
    }
    b->free_events.push_back(p.a);
    b->free_events.push_back(p.b);
  }
  b->pending.clear();
}

namespace {


int upload(void* dst, const void* src, size_t bytes, hipStream_t st) {
  PHMRF_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  return PHMRF_OK;
}

int download(void* dst, const void* src, size_t bytes, hipStream_t st) {
  PHMRF_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  return PHMRF_OK;
}


int n_stats(const phmrf_block* b) { return b->K * (1 + b->S + b->S * b->S); }

void free_family(ChainFamily& f) {
  dev_free(f.nodes);
  for (int p = 0; p < 2; ++p)
    for (int c = 0; c < 3; ++c) {
      dev_free(f.seg_start[p][c]);
      dev_free(f.seg_len[p][c]);
      f.memo[p][c] = nullptr;          // slices of phmrf_block::chain_memo
    }
}

}  // namespace

int zero_accum(phmrf_block* b, size_t first, size_t count) {
  PHMRF_HIP(hipMemsetAsync(b->accum + first, 0, count * sizeof(double), b->stream));
  return PHMRF_OK;
}


// ICM colour classes and chain families of a grid block, by direct enumeration (O(n), no sorting).
int setup_grid_tables(phmrf_block* b, const Geometry& g, int num_neighbor) {
  const int64_t n = b->n;
  const int H = g.H, W = g.W;
  // ICM colours: 2x2 parity classes (oracle/mrf_moves.icm_colours)
  {
    std::vector<int64_t> cptr(5, 0);
    for (int i = 0; i < H; ++i)
      for (int j = g.diagonal ? i : 0; j < W; ++j) ++cptr[(i % 2) * 2 + (j % 2) + 1];
    for (int c = 0; c < 4; ++c) cptr[c + 1] += cptr[c];
    std::vector<int64_t> pos(cptr.begin(), cptr.end() - 1);
    std::vector<int32_t> cnodes(n);
    for (int i = 0; i < H; ++i)
      for (int j = g.diagonal ? i : 0; j < W; ++j) cnodes[pos[(i % 2) * 2 + (j % 2)]++] = (int32_t)g.id(i, j);
    PHMRF_TRY(upload(b->colour_nodes, cnodes.data(), cnodes.size() * sizeof(int32_t), b->stream));
    b->n_colours = 4;
    b->colour_ptr = cptr;
  }
  // chain families: 0 rows, 1 columns, 2 diagonals (j - i), 3 anti-diagonals (i + j)
  for (auto& f : b->families) free_family(f);
  b->families.clear();
  const int nfam = num_neighbor == 8 ? 4 : 2;
  for (int fam = 0; fam < nfam; ++fam) {
    const int ncol = fam < 2 ? 2 : 3;
    std::vector<int32_t> order;
    order.reserve(n);
    std::vector<int32_t> chain_ptr;
    std::vector<int> chain_colour;
    auto begin_chain = [&](int key) {
      chain_ptr.push_back((int32_t)order.size());
      chain_colour.push_back(((key % ncol) + ncol) % ncol);
    };
    if (fam == 0) {
      for (int i = 0; i < H; ++i) {
        const size_t before = order.size();
        for (int j = 0; j < W; ++j)
          if (g.valid(i, j)) {
            if (order.size() == before) begin_chain(i);
            order.push_back((int32_t)g.id(i, j));
          }
      }
    } else if (fam == 1) {
      for (int j = 0; j < W; ++j) {
        const size_t before = order.size();
        for (int i = 0; i < H; ++i)
          if (g.valid(i, j)) {
            if (order.size() == before) begin_chain(j);
            order.push_back((int32_t)g.id(i, j));
          }
      }
    } else if (fam == 2) {
      for (int d = -(H - 1); d <= W - 1; ++d) {
        const size_t before = order.size();
        for (int i = std::max(0, -d); i < H && i + d < W; ++i)
          if (g.valid(i, i + d)) {
            if (order.size() == before) begin_chain(d);
            order.push_back((int32_t)g.id(i, i + d));
          }
      }
    } else {
      for (int a = 0; a <= H + W - 2; ++a) {
        const size_t before = order.size();
        for (int i = std::max(0, a - (W - 1)); i < H && i <= a; ++i)
          if (g.valid(i, a - i)) {
            if (order.size() == before) begin_chain(a);
            order.push_back((int32_t)g.id(i, a - i));
          }
      }
    }
    chain_ptr.push_back((int32_t)order.size());
    PHMRF_CHECK((int64_t)order.size() == n, PHMRF_ERR_INVALID, "internal: chain enumeration does not cover the block");
    const int C = (int)chain_ptr.size() - 1;
    int max_len = 0;
    for (int c = 0; c < C; ++c) max_len = std::max(max_len, chain_ptr[c + 1] - chain_ptr[c]);
    ChainFamily f;
    f.n_chains = C;
    f.n_colours = ncol;
    f.max_len = max_len;
    f.n_nodes = n;
    PHMRF_TRY(dev_alloc(&f.nodes, (size_t)n));
    PHMRF_TRY(upload(f.nodes, order.data(), (size_t)n * sizeof(int32_t), b->stream));
    for (int phase = 0; phase < 2; ++phase)
      for (int col = 0; col < ncol; ++col) {
        std::vector<int32_t> ss, sl;
        for (int c = 0; c < C; ++c) {
          if (chain_colour[c] != col) continue;
          const int32_t p0 = chain_ptr[c], L = chain_ptr[c + 1] - chain_ptr[c];
          // separators (fixed nodes) sit at chain positions 63, 127, ... (phase 0) or 31, 95, ... (phase 1)
          int32_t start = 0;
          int32_t sep = phase ? 31 : 63;
          while (start < L) {
            const int32_t end = std::min<int32_t>(sep, L);
            if (end > start) {
              ss.push_back(p0 + start);
              sl.push_back(end - start);
            }
            start = sep + 1;
            sep += 64;
          }
        }
        f.nseg[phase][col] = (int)ss.size();
        PHMRF_TRY(dev_alloc(&f.seg_start[phase][col], ss.size()));
        PHMRF_TRY(dev_alloc(&f.seg_len[phase][col], sl.size()));
        if (!ss.empty()) {
          PHMRF_TRY(upload(f.seg_start[phase][col], ss.data(), ss.size() * sizeof(int32_t), b->stream));
          PHMRF_TRY(upload(f.seg_len[phase][col], sl.data(), sl.size() * sizeof(int32_t), b->stream));
        }
      }
    b->families.push_back(f);
  }
  b->H = H;
  b->W = W;
  b->diagonal = g.diagonal;
  b->num_neighbor = num_neighbor;
  b->has_grid = true;
  return launch_fwd_weights(b);          // grid-native edge weights of the strip kernels
}

// ---- path moves on a graph that is no grid (round 6) ------------------------------------------------------------------
// The exact 1-D move of chain_kernel -- all K labels of <= 63 consecutive nodes, everything else fixed -- needs nothing of
// a grid but two properties of its chains: inside a chain a node's only neighbours are its predecessor and its successor
// (an INDUCED path), and chains that move at the same time share no edge.  On a general graph both are had by
// construction: a path grows from a seed at either end by a neighbour that has exactly ONE neighbour among the nodes
// already taken by this colour's paths (the end it is attached to); a seed has none.  `cnt` counts those neighbours, so a
// path is induced and two paths of a colour are never adjacent.  Colours are filled one after the other, seeds and
// extensions prefer nodes no earlier colour has covered, until every node is covered or MAX_PATH_COLOURS are full (what is
// left keeps ICM and the component moves).  Four independent decompositions (fixed seeds: the tables are the same in every
// run) fill the two cut phases of two pairs of chain families: a node meets four different paths per round pair.
// Host-side, once per graph (O(colours x edges)); general graphs are not the reference's case -- its edge builders only
// emit the contact-map stencil (utility.py:1871-2053) -- but they are what pygco.cut_general_graph accepts
// (phylo_hmrf.py:496-498).
constexpr int MAX_PATH_COLOURS = 6;          // per decomposition: two ChainFamily objects of three colours

struct PathSet {
  std::vector<int32_t> nodes;                // path after path
  std::vector<int32_t> start, len, colour;   // per path
};

static void decompose_paths(int64_t n, int D, const std::vector<int32_t>& nbr, unsigned seed, PathSet* out) {
  std::mt19937 gen(seed);
  std::vector<char> covered(n, 0), inp(n, 0);
  std::vector<int32_t> cnt(n, 0), order;
  std::vector<int32_t> path, cand;
  int64_t n_cov = 0;
  for (int colour = 0; colour < MAX_PATH_COLOURS && n_cov < n; ++colour) {
    std::fill(cnt.begin(), cnt.end(), 0);
    std::fill(inp.begin(), inp.end(), 0);
    order.clear();
    for (int64_t v = 0; v < n; ++v)
      if (!covered[v]) order.push_back((int32_t)v);
    std::shuffle(order.begin(), order.end(), gen);
    auto take = [&](int32_t v) {
      inp[v] = 1;
      const int32_t* c = &nbr[(size_t)v * D];
      for (int x = 0; x < D && c[x] >= 0; ++x) ++cnt[c[x]];
    };
    for (int32_t s0 : order) {
      if (inp[s0] || cnt[s0] != 0) continue;
      path.assign(1, s0);
      take(s0);
      for (int side = 0; side < 2; ++side) {
        while ((int)path.size() < 63) {
          const int32_t e = side == 0 ? path.back() : path.front();
          const int32_t* c = &nbr[(size_t)e * D];
          cand.clear();
          bool any_new = false;
          for (int x = 0; x < D && c[x] >= 0; ++x)
            if (!inp[c[x]] && cnt[c[x]] == 1) {
              if (!covered[c[x]] && !any_new) {
                cand.clear();
                any_new = true;
              }
              if (!any_new || !covered[c[x]]) cand.push_back(c[x]);
            }
          if (cand.empty()) break;
          const int32_t v = cand[gen() % cand.size()];
          take(v);
          if (side == 0) path.push_back(v);
          else path.insert(path.begin(), v);
        }
      }
      out->start.push_back((int32_t)out->nodes.size());
      out->len.push_back((int32_t)path.size());
      out->colour.push_back(colour);
      for (int32_t v : path) {
        out->nodes.push_back(v);
        if (!covered[v]) {
          covered[v] = 1;
          ++n_cov;
        }
      }
    }
  }
}

int setup_path_families(phmrf_block* b) {
  const int64_t n = b->n;
  const int D = b->D;
  std::vector<int32_t> nbr((size_t)n * D);
  PHMRF_TRY(download(nbr.data(), b->nbr, nbr.size() * sizeof(int32_t), b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  for (auto& f : b->families) free_family(f);
  b->families.clear();
  for (int pair = 0; pair < 2; ++pair) {                 // decompositions (2 pair, 2 pair + 1) = cut phases 0 and 1 of families 2 pair, 2 pair + 1
    PathSet ps[2];
    for (int phase = 0; phase < 2; ++phase) decompose_paths(n, D, nbr, 0x9E3779B9u + 7919u * (unsigned)(2 * pair + phase), &ps[phase]);
    for (int half = 0; half < 2; ++half) {               // colours 3 half .. 3 half + 2 of both decompositions
      ChainFamily f;
      f.n_colours = 3;
      std::vector<int32_t> order;
      std::vector<int32_t> ss[2][3], sl[2][3];
      for (int phase = 0; phase < 2; ++phase)
        for (size_t q = 0; q < ps[phase].start.size(); ++q) {
          const int col = ps[phase].colour[q] - 3 * half;
          if (col < 0 || col > 2 || ps[phase].len[q] < 2) continue;      // (a path of one node is an ICM step)
          ss[phase][col].push_back((int32_t)order.size());
          sl[phase][col].push_back(ps[phase].len[q]);
          order.insert(order.end(), ps[phase].nodes.begin() + ps[phase].start[q],
                       ps[phase].nodes.begin() + ps[phase].start[q] + ps[phase].len[q]);
          f.max_len = std::max(f.max_len, (int)ps[phase].len[q]);
          ++f.n_chains;
        }
      if (order.empty()) order.push_back(0);
      f.n_nodes = (int64_t)order.size();
      PHMRF_TRY(dev_alloc(&f.nodes, order.size()));
      PHMRF_TRY(upload(f.nodes, order.data(), order.size() * sizeof(int32_t), b->stream));
      for (int phase = 0; phase < 2; ++phase)
        for (int col = 0; col < 3; ++col) {
          f.nseg[phase][col] = (int)ss[phase][col].size();
          PHMRF_TRY(dev_alloc(&f.seg_start[phase][col], ss[phase][col].size()));
          PHMRF_TRY(dev_alloc(&f.seg_len[phase][col], sl[phase][col].size()));
          if (!ss[phase][col].empty()) {
            PHMRF_TRY(upload(f.seg_start[phase][col], ss[phase][col].data(), ss[phase][col].size() * sizeof(int32_t), b->stream));
            PHMRF_TRY(upload(f.seg_len[phase][col], sl[phase][col].data(), sl[phase][col].size() * sizeof(int32_t), b->stream));
          }
        }
      PHMRF_HIP(hipStreamSynchronize(b->stream));         // (the host vectors go out of scope)
      b->families.push_back(f);
    }
  }
  return PHMRF_OK;
}

// ---- helpers shared with the label solver (solve.hip; declared in common.h) -------------------------------------------
// strip-kernel work counters: device banks -> host totals (the stream must be synchronised by the caller afterwards)
int work_fetch_async(phmrf_block* b) {
  PHMRF_HIP(hipMemcpyAsync(b->work_host, b->work_acc, WORK_BANKS * WORK_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipMemsetAsync(b->work_acc, 0, WORK_BANKS * WORK_SLOTS * sizeof(unsigned long long), b->stream));
  return PHMRF_OK;
}
void work_fold(phmrf_block* b, bool first_round) {
  static const int SLOT_OF[WORK_SLOTS] = {0, 1, 2, 3, 5, 6, 7};   // work[4] = launches (host-counted)
  for (int k = 0; k < WORK_BANKS; ++k)
    for (int q = 0; q < WORK_SLOTS; ++q) {
      const int64_t v = (int64_t)b->work_host[k * WORK_SLOTS + q];
      b->work[SLOT_OF[q]] += v;
      if (first_round) b->work_first[SLOT_OF[q]] += v;
    }
}

int check_solvable(phmrf_block* b) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(b->has_graph, PHMRF_ERR_STATE, "graph not set");
  PHMRF_CHECK(b->has_logprob, PHMRF_ERR_STATE, "logprob not set (run phmrf_emission or phmrf_block_set_logprob)");
  return PHMRF_OK;
}

int icm_sweep_nocount(phmrf_block* b, float beta) {
  if (b->tick) ++b->tick;
  tic(b, KC_ICM);
  for (int c = 0; c < b->n_colours; ++c) PHMRF_TRY(launch_icm_colour(b, beta, c));
  toc(b, KC_ICM, b->n_colours);
  return PHMRF_OK;
}

int chain_sweep_nocount(phmrf_block* b, float beta, int family, int phase, bool timed) {
  const ChainFamily& f = b->families[family];
  if (b->tick) ++b->tick;
  if (timed) tic(b, KC_CHAIN);
  for (int c = 0; c < f.n_colours; ++c) PHMRF_TRY(launch_chain_colour(b, beta, family, c, phase));
  if (timed) toc(b, KC_CHAIN, f.n_colours);
  return PHMRF_OK;
}

// the (unary, pair without beta) sums of an energy evaluation from their two 8-byte slots: doubles, or in deterministic mode
// 2^-20 fixed-point integers (kernels.hip energy_flush)
void energy_sums(const phmrf_block* b, const void* slots, double* eu, double* ep) {
  double d[2];
  long long q[2];
  std::memcpy(d, slots, sizeof(d));
  std::memcpy(q, slots, sizeof(q));
  *eu = b->deterministic ? (double)q[0] / 1048576.0 : d[0];
  *ep = b->deterministic ? (double)q[1] / 1048576.0 : d[1];
}

int energy_now(phmrf_block* b, double beta, double* eu, double* ep) {
  PHMRF_TRY(zero_accum(b, 4, 2));
  tic(b, KC_ENERGY);
  PHMRF_TRY(launch_energy(b, (float)beta));
  toc(b, KC_ENERGY, 1);
  PHMRF_HIP(hipMemcpyAsync(b->accum_host + 4, b->accum + 4, 2 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  energy_sums(b, b->accum_host + 4, eu, ep);
  *ep = beta * *ep;
  return PHMRF_OK;
}

int strip_pass_nocount(phmrf_block* b, float beta, int orient, int shift_r, int shift_c, int alpha, int geom, bool timed) {
  if (!b->uT_valid) {                       // (before the proposals: on a grid they are formed from the planes)
    tic(b, KC_PROPOSE);
    PHMRF_TRY(launch_unary_planes(b));
    toc(b, KC_PROPOSE, 1);
  }
  if (alpha < 0) {
    tic(b, KC_PROPOSE);
    PHMRF_TRY(launch_propose(b, beta));
    toc(b, KC_PROPOSE, 1);
  }
  if (timed) tic(b, KC_FUSION);
  if (b->tick) ++b->tick;
  PHMRF_TRY(launch_strip_pass(b, beta, orient, shift_r, shift_c, alpha, geom));
  b->work[4] += 1;
  if (timed) toc(b, KC_FUSION, 1);
  return PHMRF_OK;
}

}  // namespace phmrf

using namespace phmrf;

extern "C" {

// ---- library ------------------------------------------------------------------------------------
int phmrf_version(void) { return PHMRF_VERSION; }

const char* phmrf_last_error(void) { return g_error.c_str(); }

const char* phmrf_status_string(int status) {
  switch (status) {
    case PHMRF_OK: return "ok";
    case PHMRF_ERR_INVALID: return "invalid argument";
    case PHMRF_ERR_HIP: return "HIP runtime error";
    case PHMRF_ERR_NO_DEVICE: return "no GPU device";
    case PHMRF_ERR_UNSUPPORTED: return "unsupported configuration";
    case PHMRF_ERR_STATE: return "call order / missing input";
    case PHMRF_ERR_NOT_PD: return "covariance not positive definite";
  }
  return "unknown status";
}

int phmrf_device_count(int* count) {
  PHMRF_CHECK(count, PHMRF_ERR_INVALID, "count is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    return fail(PHMRF_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = c;
  return PHMRF_OK;
}

int phmrf_set_device(int device) {
  PHMRF_HIP(hipSetDevice(device));
  return PHMRF_OK;
}

// ---- block lifetime -----------------------------------------------------------------------------
static bool deterministic_env() {       // PHMRF_DETERMINISTIC=1: order-independent reductions (read at every block creation)
  const char* e = getenv("PHMRF_DETERMINISTIC");
  return e && e[0] == '1';
}

int phmrf_block_create(int64_t n, int S, int K, phmrf_block_t* out) {
  PHMRF_CHECK(out, PHMRF_ERR_INVALID, "out is NULL");
  *out = nullptr;
  PHMRF_CHECK(n > 0 && n < ((int64_t)1 << 31) - 64, PHMRF_ERR_INVALID, "n must be in [1, 2^31)");
  PHMRF_CHECK(S >= 1 && S <= 16, PHMRF_ERR_UNSUPPORTED, "S must be in [1,16]");
  PHMRF_CHECK(K >= 1 && K <= 64, PHMRF_ERR_UNSUPPORTED, "K must be in [1,64]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PHMRF_ERR_NO_DEVICE, "no HIP device visible");
  phmrf_block* b = new phmrf_block();
  b->n = n;
  b->S = S;
  b->K = K;
  b->deterministic = deterministic_env();
  int st = PHMRF_OK;
  auto guard = [&](int s) {
    if (s != PHMRF_OK && st == PHMRF_OK) st = s;
  };
  if (hipGetDevice(&b->device) != hipSuccess) guard(fail(PHMRF_ERR_HIP, "hipGetDevice failed"));
  if (st == PHMRF_OK && hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking) != hipSuccess)
    guard(fail(PHMRF_ERR_HIP, "hipStreamCreate failed"));
  b->stream = b->own_stream;
  if (st == PHMRF_OK) guard(dev_alloc(&b->X, (size_t)n * S));
  if (st == PHMRF_OK) guard(dev_alloc(&b->logprob, (size_t)n * K));
  if (st == PHMRF_OK) guard(dev_alloc(&b->labels, (size_t)n));
  if (st == PHMRF_OK) guard(dev_alloc(&b->labels_tmp, (size_t)n));
  if (st == PHMRF_OK) guard(dev_alloc(&b->accum, (size_t)ACCUM_DOUBLES));
  if (st == PHMRF_OK) guard(dev_alloc(&b->counters, (size_t)N_COUNTERS));
  if (st == PHMRF_OK) guard(dev_alloc(&b->work_acc, (size_t)WORK_BANKS * WORK_SLOTS));
  if (st == PHMRF_OK && hipMemsetAsync(b->work_acc, 0, WORK_BANKS * WORK_SLOTS * sizeof(unsigned long long), b->own_stream) != hipSuccess)
    guard(fail(PHMRF_ERR_HIP, "hipMemset failed"));
  if (st == PHMRF_OK && hipHostMalloc(reinterpret_cast<void**>(&b->work_host), WORK_BANKS * WORK_SLOTS * sizeof(unsigned long long)) != hipSuccess)
    guard(fail(PHMRF_ERR_HIP, "hipHostMalloc failed"));
  if (st == PHMRF_OK) guard(dev_alloc(&b->emis_params, (size_t)K * (S + S * (S + 1) / 2 + 1)));
  if (st == PHMRF_OK && hipHostMalloc(reinterpret_cast<void**>(&b->accum_host), ACCUM_DOUBLES * sizeof(double)) != hipSuccess)
    guard(fail(PHMRF_ERR_HIP, "hipHostMalloc failed"));
  if (st == PHMRF_OK && hipHostMalloc(reinterpret_cast<void**>(&b->counters_host), N_COUNTERS * sizeof(unsigned long long)) != hipSuccess)
    guard(fail(PHMRF_ERR_HIP, "hipHostMalloc failed"));
  if (st == PHMRF_OK && (hipEventCreate(&b->ev0) != hipSuccess || hipEventCreate(&b->ev1) != hipSuccess))
    guard(fail(PHMRF_ERR_HIP, "hipEventCreate failed"));
  if (st == PHMRF_OK && hipMemsetAsync(b->labels, 0, (size_t)n, b->stream) != hipSuccess)
    guard(fail(PHMRF_ERR_HIP, "hipMemset failed"));
  if (st != PHMRF_OK) {
    std::string keep = g_error;
    phmrf_block_destroy(b);
    g_error = keep;
    return st;
  }
  *out = b;
  return PHMRF_OK;
}

int phmrf_block_destroy(phmrf_block_t b) {
  if (!b) return PHMRF_OK;
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  coarse_children_destroy(b);
  if (b->c2f) {
    (void)phmrf_block_destroy(b->c2f);
    b->c2f = nullptr;
  }
  dev_free(b->X);
  dev_free(b->logprob);
  dev_free(b->labels);
  dev_free(b->labels_tmp);
  dev_free(b->labels_eval);
  dev_free(b->coarse_flag);
  dev_free(b->coarse_lab);
  if (b->coarse_lab_host) (void)hipHostFree(b->coarse_lab_host);
  b->coarse_lab_host = nullptr;
  dev_free(b->sgain);
  dev_free(b->mf_rev);
  dev_free(b->mf_theta);
  dev_free(b->mf_cap);
  dev_free(b->mf_tcap);
  dev_free(b->mf_exc);
  dev_free(b->mf_hgt);
  dev_free(b->mf_flags);
  if (b->mf_flags_host) (void)hipHostFree(b->mf_flags_host);
  b->mf_flags_host = nullptr;
  for (int s = 0; s < 4; ++s) dev_free(b->saved[s]);
  dev_free(b->nbr);
  dev_free(b->wgt);
  dev_free(b->colour_nodes);
  for (auto& f : b->families) free_family(f);
  dev_free(b->comp);
  dev_free(b->comp_tab);
  dev_free(b->comp_tab64);
  dev_free(b->post_partial);
  dev_free(b->comp_best);
  dev_free(b->comp_gain);
  dev_free(b->cc_seen);
  dev_free(b->cc_stale);
  dev_free(b->stamp);
  dev_free(b->memo);
  dev_free(b->chain_memo);
  dev_free(b->fwd_w);
  if (b->uT_raw) {                          // (the planes own their allocation; a coarse child's live in its parent's arena)
    dev_free(b->uT_raw);
    b->uT = nullptr;
  }
  dev_free(b->emis_params);
  dev_free(b->posteriors);
  dev_free(b->summary);
  dev_free(b->anc);
  for (int r = 0; r < 2; ++r) {
    dev_free(b->pin_save[r]);
    dev_free(b->pin_label[r]);
  }
  dev_free(b->xfer);
  if (b->xfer_host) (void)hipHostFree(b->xfer_host);
  if (b->ss) {
    delete b->ss;
    b->ss = nullptr;
  }
  dev_free(b->accum);
  dev_free(b->counters);
  dev_free(b->work_acc);
  if (b->work_host) (void)hipHostFree(b->work_host);
  if (b->accum_host) (void)hipHostFree(b->accum_host);
  if (b->counters_host) (void)hipHostFree(b->counters_host);
  for (auto& p : b->pending) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  for (auto e : b->free_events) (void)hipEventDestroy(e);
  if (b->cur_start) (void)hipEventDestroy(b->cur_start);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return PHMRF_OK;
}

int phmrf_block_set_stream(phmrf_block_t b, void* hip_stream) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  b->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : b->own_stream;
  for (int lv = 0; lv < N_COARSE_CHILDREN; ++lv)
    if (b->coarse[lv]) b->coarse[lv]->stream = b->stream;
  return PHMRF_OK;
}

int phmrf_block_sync(phmrf_block_t b) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  return PHMRF_OK;
}

int phmrf_block_set_observations(phmrf_block_t b, const double* X) {
  PHMRF_CHECK(b && X, PHMRF_ERR_INVALID, "NULL argument");
  const size_t cnt = (size_t)b->n * b->S;
  std::vector<float> tmp(cnt);
  for (size_t i = 0; i < cnt; ++i) tmp[i] = (float)X[i];
  PHMRF_TRY(upload(b->X, tmp.data(), cnt * sizeof(float), b->stream));
  b->has_X = true;
  return PHMRF_OK;
}

int phmrf_block_set_observations_dev(phmrf_block_t b, const float* X_dev) {
  PHMRF_CHECK(b && X_dev, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_HIP(hipMemcpyAsync(b->X, X_dev, (size_t)b->n * b->S * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
  b->has_X = true;
  return PHMRF_OK;
}

// ---- graph --------------------------------------------------------------------------------------
int phmrf_block_set_graph(phmrf_block_t b, int64_t E, const int64_t* edges, const double* w) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(E >= 0 && (E == 0 || (edges && w)), PHMRF_ERR_INVALID, "edges / w is NULL");
  const int64_t n = b->n;
  std::vector<int32_t> deg(n, 0);
  for (int64_t e = 0; e < E; ++e) {
    const int64_t a = edges[2 * e], c = edges[2 * e + 1];
    PHMRF_CHECK(a >= 0 && a < n && c >= 0 && c < n, PHMRF_ERR_INVALID, "edge endpoint out of range");
    PHMRF_CHECK(a != c, PHMRF_ERR_INVALID, "self loop in edge list");
    PHMRF_CHECK(w[e] >= 0.0 && std::isfinite(w[e]), PHMRF_ERR_INVALID, "edge weights must be finite and >= 0");
    ++deg[a];
    ++deg[c];
  }
  int maxdeg = 0;
  for (int64_t i = 0; i < n; ++i) maxdeg = std::max(maxdeg, deg[i]);
  PHMRF_CHECK(maxdeg <= 64, PHMRF_ERR_UNSUPPORTED, "node degree > 64 is not supported");
  const int D = std::max(4, (maxdeg + 3) / 4 * 4);
  std::vector<int32_t> nbr((size_t)n * D, -1);
  std::vector<float> wgt((size_t)n * D, 0.f);
  std::fill(deg.begin(), deg.end(), 0);
  for (int64_t e = 0; e < E; ++e) {
    const int64_t a = edges[2 * e], c = edges[2 * e + 1];
    nbr[(size_t)a * D + deg[a]] = (int32_t)c;
    wgt[(size_t)a * D + deg[a]++] = (float)w[e];
    nbr[(size_t)c * D + deg[c]] = (int32_t)a;
    wgt[(size_t)c * D + deg[c]++] = (float)w[e];
  }
  // neighbours ascending (deterministic summation order == oracle/mrf_moves.Graph); rows are short
  for (int64_t i = 0; i < n; ++i) {
    int32_t* c = &nbr[(size_t)i * D];
    float* ww = &wgt[(size_t)i * D];
    for (int x = 1; x < deg[i]; ++x) {
      const int32_t cv = c[x];
      const float wv = ww[x];
      int y = x - 1;
      while (y >= 0 && c[y] > cv) {
        c[y + 1] = c[y];
        ww[y + 1] = ww[y];
        --y;
      }
      c[y + 1] = cv;
      ww[y + 1] = wv;
    }
    for (int x = 1; x < deg[i]; ++x)
      PHMRF_CHECK(c[x] != c[x - 1], PHMRF_ERR_INVALID, "duplicate edge in edge list");
  }
  // greedy colouring in index order (replaced by the parity colouring when a grid is declared)
  std::vector<int32_t> colour(n, -1);
  int ncol = 0;
  {
    std::vector<int> mark(66, -1);
    for (int64_t i = 0; i < n; ++i) {
      const int32_t* c = &nbr[(size_t)i * D];
      for (int x = 0; x < deg[i]; ++x)
        if (colour[c[x]] >= 0) mark[colour[c[x]]] = (int)(i & 0x7fffffff);
      int col = 0;
      while (mark[col] == (int)(i & 0x7fffffff)) ++col;
      colour[i] = col;
      ncol = std::max(ncol, col + 1);
    }
  }
  std::vector<int64_t> cptr(ncol + 1, 0);
  for (int64_t i = 0; i < n; ++i) ++cptr[colour[i] + 1];
  for (int c = 0; c < ncol; ++c) cptr[c + 1] += cptr[c];
  std::vector<int32_t> cnodes(n);
  {
    std::vector<int64_t> pos(cptr.begin(), cptr.end() - 1);
    for (int64_t i = 0; i < n; ++i) cnodes[pos[colour[i]]++] = (int32_t)i;
  }
  dev_free(b->nbr);
  dev_free(b->wgt);
  dev_free(b->colour_nodes);
  PHMRF_TRY(dev_alloc(&b->nbr, (size_t)n * D));
  PHMRF_TRY(dev_alloc(&b->wgt, (size_t)n * D));
  PHMRF_TRY(dev_alloc(&b->colour_nodes, (size_t)n));
  PHMRF_TRY(upload(b->nbr, nbr.data(), nbr.size() * sizeof(int32_t), b->stream));
  PHMRF_TRY(upload(b->wgt, wgt.data(), wgt.size() * sizeof(float), b->stream));
  PHMRF_TRY(upload(b->colour_nodes, cnodes.data(), cnodes.size() * sizeof(int32_t), b->stream));
  b->D = D;
  b->E = E;
  b->n_colours = ncol;
  b->colour_ptr = cptr;
  b->has_graph = true;
  b->has_grid = false;
  for (auto& f : b->families) free_family(f);
  b->families.clear();
  dev_free(b->mf_rev);                       // (the arcs' reverse slots and the flow's arrays belong to the old graph)
  dev_free(b->mf_theta);
  dev_free(b->mf_cap);
  dev_free(b->mf_tcap);
  dev_free(b->mf_exc);
  dev_free(b->mf_hgt);
  return PHMRF_OK;
}

int phmrf_block_set_grid(phmrf_block_t b, int H, int W, int diagonal, int num_neighbor) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(b->has_graph, PHMRF_ERR_STATE, "set_graph must precede set_grid");
  PHMRF_CHECK(H >= 1 && W >= 1, PHMRF_ERR_INVALID, "H, W must be >= 1");
  PHMRF_CHECK(num_neighbor == 8 || num_neighbor == 4, PHMRF_ERR_INVALID, "num_neighbor must be 8 or 4");
  PHMRF_CHECK(!diagonal || H <= W, PHMRF_ERR_INVALID, "a diagonal block is the first H <= W rows of a W x W upper triangle");
  Geometry g(H, W, diagonal);
  PHMRF_CHECK(g.count() == b->n, PHMRF_ERR_INVALID, "H, W, diagonal do not match the node count");
  const int64_t n = b->n;
  const int D = b->D;
  std::vector<int32_t> nbr((size_t)n * D);
  std::vector<float> wgt((size_t)n * D);
  PHMRF_TRY(download(nbr.data(), b->nbr, nbr.size() * sizeof(int32_t), b->stream));
  PHMRF_TRY(download(wgt.data(), b->wgt, wgt.size() * sizeof(float), b->stream));
  std::vector<int32_t> ci(n), cj(n);
  for (int64_t v = 0; v < n; ++v) {
    int i, j;
    g.coords(v, &i, &j);
    ci[v] = i;
    cj[v] = j;
  }
  int64_t present = 0, expected = 0;       // adjacency entries on file / entries of the complete stencil
  for (int64_t v = 0; v < n; ++v) {
    for (int x = 0; x < D; ++x) {
      const int32_t u = nbr[(size_t)v * D + x];
      if (u < 0) continue;
      const int di = std::abs(ci[u] - ci[v]), dj = std::abs(cj[u] - cj[v]);
      PHMRF_CHECK(di <= 1 && dj <= 1 && (di + dj) > 0, PHMRF_ERR_INVALID, "edge list joins nodes that are not grid neighbours");
      PHMRF_CHECK(num_neighbor == 8 || (di + dj) == 1, PHMRF_ERR_INVALID, "diagonal edge in a 4-neighbour block");
      ++present;
    }
    for (int di = -1; di <= 1; ++di)
      for (int dj = -1; dj <= 1; ++dj) {
        if ((di == 0 && dj == 0) || (num_neighbor == 4 && di != 0 && dj != 0)) continue;
        const int ni = ci[v] + di, nj = cj[v] + dj;
        if (ni < 0 || ni >= H || nj < 0 || nj >= W || (diagonal && ni > nj)) continue;
        ++expected;
      }
  }
  PHMRF_TRY(setup_grid_tables(b, g, num_neighbor));
  // An edge list that is a subset of the stencil is accepted.  Whatever reads WEIGHTS is indifferent to a missing edge (it
  // weighs 0: the forward-edge records of the strip, coarse and table kernels, the chain links, the adjacency rows).  What
  // reasons from the SHAPE of the stencil is switched off by grid_complete = false: the component kernels by geometry and
  // the stencil shortcut of cc_union_kernel (a linked-left node leaving unions to its run-mate: launch_cc runs the
  // adjacency-row kernels without it), and the kernels that COUNT their neighbours by geometry (the posterior kernel:
  // isolated nodes, estimate_type != 3).
  b->grid_complete = present == expected;
  return PHMRF_OK;
}

int phmrf_block_build_grid_graph(phmrf_block_t b, int H, int W, int diagonal, int num_neighbor, double beta1) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(b->has_X, PHMRF_ERR_STATE, "observations must be set before the graph is built from them");
  PHMRF_CHECK(H >= 1 && W >= 1, PHMRF_ERR_INVALID, "H, W must be >= 1");
  PHMRF_CHECK(num_neighbor == 8 || num_neighbor == 4, PHMRF_ERR_INVALID, "num_neighbor must be 8 or 4");
  PHMRF_CHECK(!diagonal || H <= W, PHMRF_ERR_INVALID, "a diagonal block is the first H <= W rows of a W x W upper triangle");
  PHMRF_CHECK(beta1 >= 0.0 && std::isfinite(beta1), PHMRF_ERR_INVALID, "beta1 must be finite and >= 0");
  Geometry g(H, W, diagonal);
  PHMRF_CHECK(g.count() == b->n, PHMRF_ERR_INVALID, "H, W, diagonal do not match the node count");
  dev_free(b->nbr);
  dev_free(b->wgt);
  PHMRF_TRY(dev_alloc(&b->nbr, (size_t)b->n * 8));
  PHMRF_TRY(dev_alloc(&b->wgt, (size_t)b->n * 8));
  b->D = 8;
  PHMRF_TRY(launch_grid_graph(b, H, W, diagonal, num_neighbor, beta1));
  if (!b->colour_nodes) PHMRF_TRY(dev_alloc(&b->colour_nodes, (size_t)b->n));
  b->has_graph = true;
  b->E = 0;
  PHMRF_TRY(setup_grid_tables(b, g, num_neighbor));
  b->grid_complete = true;                 // built from the stencil: every edge is there
  return PHMRF_OK;
}

int phmrf_block_get_adjacency(phmrf_block_t b, int* D, int32_t* nbr_out, float* wgt_out) {
  PHMRF_CHECK(b && D, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(b->has_graph, PHMRF_ERR_STATE, "graph not set");
  *D = b->D;
  if (nbr_out) PHMRF_TRY(download(nbr_out, b->nbr, (size_t)b->n * b->D * sizeof(int32_t), b->stream));
  if (wgt_out) PHMRF_TRY(download(wgt_out, b->wgt, (size_t)b->n * b->D * sizeof(float), b->stream));
  return PHMRF_OK;
}

// ---- labels -------------------------------------------------------------------------------------
int phmrf_block_set_labels(phmrf_block_t b, const int32_t* labels) {
  PHMRF_CHECK(b && labels, PHMRF_ERR_INVALID, "NULL argument");
  std::vector<uint8_t> tmp(b->n);
  for (int64_t i = 0; i < b->n; ++i) {
    PHMRF_CHECK(labels[i] >= 0 && labels[i] < b->K, PHMRF_ERR_INVALID, "label out of range [0,K)");
    tmp[i] = (uint8_t)labels[i];
  }
  PHMRF_TRY(upload(b->labels, tmp.data(), (size_t)b->n, b->stream));
  b->has_labels = true;
  b->labels_are_slot = 0;
  return PHMRF_OK;
}

static int fetch_labels(phmrf_block_t b, const uint8_t* src, int32_t* labels) {
  std::vector<uint8_t> tmp(b->n);
  PHMRF_TRY(download(tmp.data(), src, (size_t)b->n, b->stream));
  for (int64_t i = 0; i < b->n; ++i) labels[i] = tmp[i];
  return PHMRF_OK;
}

int phmrf_block_get_labels(phmrf_block_t b, int32_t* labels) {
  PHMRF_CHECK(b && labels, PHMRF_ERR_INVALID, "NULL argument");
  return fetch_labels(b, b->labels, labels);
}

int phmrf_block_save_labels(phmrf_block_t b, int slot) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(slot >= 0 && slot < 4, PHMRF_ERR_INVALID, "slot must be in [0,4)");
  if (!b->saved[slot]) PHMRF_TRY(dev_alloc(&b->saved[slot], (size_t)b->n));
  PHMRF_HIP(hipMemcpyAsync(b->saved[slot], b->labels, (size_t)b->n, hipMemcpyDeviceToDevice, b->stream));
  b->labels_are_slot |= 1 << slot;
  return PHMRF_OK;
}

int phmrf_block_restore_labels(phmrf_block_t b, int slot) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(slot >= 0 && slot < 4 && b->saved[slot], PHMRF_ERR_STATE, "label slot is empty");
  PHMRF_HIP(hipMemcpyAsync(b->labels, b->saved[slot], (size_t)b->n, hipMemcpyDeviceToDevice, b->stream));
  b->has_labels = true;
  b->labels_are_slot = 1 << slot;
  return PHMRF_OK;
}

int phmrf_block_get_saved_labels(phmrf_block_t b, int slot, int32_t* labels) {
  PHMRF_CHECK(b && labels, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(slot >= 0 && slot < 4 && b->saved[slot], PHMRF_ERR_STATE, "label slot is empty");
  return fetch_labels(b, b->saved[slot], labels);
}

// ---- b1 emission --------------------------------------------------------------------------------
int phmrf_emission_pack_size(int S, int K, int64_t* n_floats) {
  PHMRF_CHECK(n_floats && S >= 1 && S <= 16 && K >= 1, PHMRF_ERR_INVALID, "bad S/K");
  *n_floats = (int64_t)K * (S + S * (S + 1) / 2 + 1);
  return PHMRF_OK;
}

int phmrf_emission_pack(int S, int K, const double* means, const double* covars, float* packed) {
  PHMRF_CHECK(means && covars && packed, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(S >= 1 && S <= 16 && K >= 1, PHMRF_ERR_INVALID, "bad S/K");
  const int PS = S + S * (S + 1) / 2 + 1;
  std::vector<double> L(S * S), Li(S * S);
  for (int k = 0; k < K; ++k) {
    const double* cv = covars + (size_t)k * S * S;
    bool ok = false;
    for (int attempt = 0; attempt < 2 && !ok; ++attempt) {  // sklearn 0.18: retry once with +1e-7*I
      const double jitter = attempt ? 1e-7 : 0.0;
      ok = true;
      std::fill(L.begin(), L.end(), 0.0);
      for (int i = 0; i < S && ok; ++i)
        for (int j = 0; j <= i; ++j) {
          double s = cv[i * S + j] + (i == j ? jitter : 0.0);
          for (int t = 0; t < j; ++t) s -= L[i * S + t] * L[j * S + t];
          if (i == j) {
            if (!(s > 0.0) || !std::isfinite(s)) { ok = false; break; }
            L[i * S + i] = std::sqrt(s);
          } else {
            L[i * S + j] = s / L[j * S + j];
          }
        }
    }
    if (!ok) return fail(PHMRF_ERR_NOT_PD, "'covars' must be symmetric, positive-definite (state " + std::to_string(k) + ")");
    // Li = L^-1 (lower) by forward substitution; logdet = 2 sum log diag(L)
    std::fill(Li.begin(), Li.end(), 0.0);
    double logdet = 0.0;
    for (int i = 0; i < S; ++i) logdet += 2.0 * std::log(L[i * S + i]);
    for (int c = 0; c < S; ++c)
      for (int i = c; i < S; ++i) {
        double s = (i == c) ? 1.0 : 0.0;
        for (int t = c; t < i; ++t) s -= L[i * S + t] * Li[t * S + c];
        Li[i * S + c] = s / L[i * S + i];
      }
    float* p = packed + (size_t)k * PS;
    for (int s = 0; s < S; ++s) p[s] = (float)means[(size_t)k * S + s];
    int idx = S;
    for (int i = 0; i < S; ++i)
      for (int c = 0; c <= i; ++c) p[idx++] = (float)Li[i * S + c];
    p[idx] = (float)(-0.5 * (S * std::log(2.0 * M_PI) + logdet));
  }
  return PHMRF_OK;
}

int phmrf_emission_dev(const float* X_dev, int64_t n, int S, int K, const float* packed_dev, float* logprob_dev,
                       void* hip_stream) {
  PHMRF_CHECK(X_dev && packed_dev && logprob_dev, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(n > 0 && K >= 1 && K <= 64, PHMRF_ERR_INVALID, "bad n/K");
  return launch_emission(X_dev, n, S, K, packed_dev, logprob_dev, nullptr, reinterpret_cast<hipStream_t>(hip_stream));
}

int phmrf_emission(phmrf_block_t b, const double* means, const double* covars) {
  PHMRF_CHECK(b && means && covars, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(b->has_X, PHMRF_ERR_STATE, "observations not set");
  const int PS = b->S + b->S * (b->S + 1) / 2 + 1;
  std::vector<float> packed((size_t)b->K * PS);
  PHMRF_TRY(phmrf_emission_pack(b->S, b->K, means, covars, packed.data()));
  PHMRF_TRY(upload(b->emis_params, packed.data(), packed.size() * sizeof(float), b->stream));
  tic(b, KC_EMISSION);
  // (a block that has run strip moves before owns its unary planes: the kernel writes them along with logprob)
  PHMRF_TRY(launch_emission(b->X, b->n, b->S, b->K, b->emis_params, b->logprob, b->uT, b->stream));
  toc(b, KC_EMISSION, 1);
  b->has_logprob = true;
  b->uT_valid = b->uT != nullptr;
  b->pin_saved = false;                     // (every row is real again: whatever was pinned is not any more)
  b->pin_rows[0] = b->pin_rows[1] = 0;
  return PHMRF_OK;
}

int phmrf_block_get_logprob(phmrf_block_t b, double* logprob) {
  PHMRF_CHECK(b && logprob, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(b->has_logprob, PHMRF_ERR_STATE, "logprob not computed");
  const size_t cnt = (size_t)b->n * b->K;
  std::vector<float> tmp(cnt);
  PHMRF_TRY(download(tmp.data(), b->logprob, cnt * sizeof(float), b->stream));
  for (size_t i = 0; i < cnt; ++i) logprob[i] = tmp[i];
  return PHMRF_OK;
}

int phmrf_block_set_logprob(phmrf_block_t b, const double* logprob) {
  PHMRF_CHECK(b && logprob, PHMRF_ERR_INVALID, "NULL argument");
  const size_t cnt = (size_t)b->n * b->K;
  std::vector<float> tmp(cnt);
  for (size_t i = 0; i < cnt; ++i) tmp[i] = (float)logprob[i];
  PHMRF_TRY(upload(b->logprob, tmp.data(), cnt * sizeof(float), b->stream));
  b->has_logprob = true;
  b->uT_valid = false;
  b->pin_saved = false;
  b->pin_rows[0] = b->pin_rows[1] = 0;
  return PHMRF_OK;
}

// ---- b2 MRF -------------------------------------------------------------------------------------
// the single-pass entry points count into COUNTER_DEFAULT
static int read_counter(phmrf_block_t b, int64_t* v) {      // (v may be NULL: the wait is the same)
  PHMRF_HIP(hipMemcpyAsync(b->counters_host + COUNTER_DEFAULT, b->counters + COUNTER_DEFAULT, sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  if (v) *v = (int64_t)b->counters_host[COUNTER_DEFAULT];
  return PHMRF_OK;
}

static int zero_counter(phmrf_block_t b) {
  PHMRF_HIP(hipMemsetAsync(b->counters, 0, N_COUNTERS * sizeof(unsigned long long), b->stream));
  b->counter_slot = COUNTER_DEFAULT;
  return PHMRF_OK;
}

int phmrf_mrf_energy(phmrf_block_t b, double beta, double* e_total, double* e_unary, double* e_pair) {
  PHMRF_TRY(check_solvable(b));
  double eu, ep;
  PHMRF_TRY(energy_now(b, beta, &eu, &ep));
  if (e_total) *e_total = eu + ep;
  if (e_unary) *e_unary = eu;
  if (e_pair) *e_pair = ep;
  return PHMRF_OK;
}

// The warm start of an E-step.  The reference starts every labelling from labels_local, the labels of the EM iteration with
// the lowest cost so far (phylo_hmrf.py:479, base.py:416-420) -- which can be many iterations old: the start is then far
// from any minimum of the energy under the current parameters and the solve pays for a cold start.  The block's CURRENT
// labels are the previous E-step's result; both candidates are scored under the logprob that is resident now and the lower
// energy wins.  choose = 0: only score (the tiles of a split block decide on their sums).
int phmrf_block_warm_start(phmrf_block_t b, double beta, int slot, int choose, double* e_current, double* e_saved, int* took_saved) {
  PHMRF_TRY(check_solvable(b));
  PHMRF_CHECK(slot >= 0 && slot < 4 && b->saved[slot], PHMRF_ERR_STATE, "label slot is empty");
  if (took_saved) *took_saved = 1;
  const bool report = e_current || e_saved || took_saved;
  if (!b->has_labels || ((b->labels_are_slot >> slot) & 1)) {        // nothing to compare with / the snapshot IS the current labelling
    if (choose && !b->has_labels) PHMRF_TRY(phmrf_block_restore_labels(b, slot));
    if (e_current) *e_current = std::numeric_limits<double>::infinity();
    if (e_saved) *e_saved = 0.0;
    return PHMRF_OK;
  }
  double* const extra = b->accum + (ACCUM_DOUBLES - 4);     // (behind every statistic the accum area can hold)
  if (choose && !report && b->n >= (1 << 16) && energy_diff_available(b)) {
    // nobody asked for the two energies: what decides is the SIGN of their difference, which comes from the nodes where the
    // two labellings differ (energy_diff_grid_kernel) -- one light pass instead of two full ones; the choice kernel then
    // compares (difference, 0)
    PHMRF_TRY(zero_accum(b, 4, 2));
    PHMRF_TRY(zero_accum(b, ACCUM_DOUBLES - 4, 2));
    tic(b, KC_ENERGY);
    PHMRF_TRY(launch_energy_diff(b, b->saved[slot]));
    PHMRF_TRY(launch_choose_labels(b, b->saved[slot], b->accum + 4, extra, beta));
    toc(b, KC_ENERGY, 2);
    b->labels_are_slot = 0;
    return PHMRF_OK;
  }
  // the two evaluations and the choice are queued on the block's stream; the host waits only if it wants the numbers
  PHMRF_TRY(zero_accum(b, 4, 2));
  PHMRF_TRY(zero_accum(b, ACCUM_DOUBLES - 4, 2));
  tic(b, KC_ENERGY);
  PHMRF_TRY(launch_energy(b, (float)beta));
  std::swap(b->labels, b->saved[slot]);                     // (score the snapshot in place)
  const int st = launch_energy(b, (float)beta, extra);
  std::swap(b->labels, b->saved[slot]);
  PHMRF_TRY(st);
  if (choose) PHMRF_TRY(launch_choose_labels(b, b->saved[slot], b->accum + 4, extra, beta));
  toc(b, KC_ENERGY, choose ? 3 : 2);
  if (choose) b->labels_are_slot = 0;
  if (!report) return PHMRF_OK;
  PHMRF_HIP(hipMemcpyAsync(b->accum_host + 4, b->accum + 4, 2 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipMemcpyAsync(b->accum_host + 6, extra, 2 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  double ec[2], es[2];
  energy_sums(b, b->accum_host + 4, &ec[0], &ec[1]);
  energy_sums(b, b->accum_host + 6, &es[0], &es[1]);
  const double cur = ec[0] + beta * ec[1], sav = es[0] + beta * es[1];
  if (e_current) *e_current = cur;
  if (e_saved) *e_saved = sav;
  if (took_saved) *took_saved = !(cur < sav) ? 1 : 0;
  return PHMRF_OK;
}

// E(current labels) - E(snapshot) as a number, from the nodes where the two differ: the kernel behind the unreported warm
// start, at any size (the size gate is phmrf_block_warm_start's own).  Never another way: where the kernel cannot run the
// call says so.
int phmrf_block_energy_diff(phmrf_block_t b, double beta, int slot, double* out) {
  PHMRF_TRY(check_solvable(b));
  PHMRF_CHECK(out, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(slot >= 0 && slot < 4 && b->saved[slot], PHMRF_ERR_STATE, "label slot is empty");
  PHMRF_CHECK(b->has_labels, PHMRF_ERR_STATE, "labels not set");
  PHMRF_CHECK(b->has_grid && b->fwd_w && b->H > 0 && b->W > 0, PHMRF_ERR_UNSUPPORTED,
              "the energy difference from the differing nodes needs a grid block (phmrf_block_set_grid / build_grid_graph)");
  PHMRF_CHECK(energy_diff_available(b), PHMRF_ERR_STATE,
              "the unary planes are not current (a strip pass or a solve builds them after phmrf_block_set_logprob)");
  PHMRF_TRY(zero_accum(b, 4, 2));
  tic(b, KC_ENERGY);
  PHMRF_TRY(launch_energy_diff(b, b->saved[slot]));
  toc(b, KC_ENERGY, 1);
  PHMRF_HIP(hipMemcpyAsync(b->accum_host + 4, b->accum + 4, 2 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  energy_sums(b, b->accum_host + 4, &out[0], &out[1]);
  out[1] = beta * out[1];
  return PHMRF_OK;
}

int phmrf_mrf_icm_sweep(phmrf_block_t b, double beta, int64_t* changed) {
  PHMRF_TRY(check_solvable(b));
  b->labels_are_slot = 0;
  PHMRF_TRY(zero_counter(b));
  PHMRF_TRY(icm_sweep_nocount(b, (float)beta));
  return read_counter(b, changed);
}

// a graph without grid geometry gets its path families at its first use, as at its first solve (solve.hip)
static int ensure_chain_families(phmrf_block* b) {
  if (!b->has_grid && b->families.empty() && b->nbr && b->n >= 2) PHMRF_TRY(setup_path_families(b));
  return PHMRF_OK;
}

int phmrf_mrf_chain_sweep(phmrf_block_t b, double beta, int family, int64_t* changed) {
  PHMRF_TRY(check_solvable(b));
  b->labels_are_slot = 0;
  PHMRF_TRY(ensure_chain_families(b));
  PHMRF_CHECK(family >= 0 && family < (int)b->families.size(), PHMRF_ERR_INVALID, "no such chain family");
  PHMRF_TRY(zero_counter(b));
  PHMRF_TRY(chain_sweep_nocount(b, (float)beta, family, 0));
  PHMRF_TRY(chain_sweep_nocount(b, (float)beta, family, 1));
  return read_counter(b, changed);
}

int phmrf_block_chain_family_info(phmrf_block_t b, int* n_families, int* n_colours) {
  PHMRF_CHECK(b && n_families, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(b->has_graph, PHMRF_ERR_STATE, "graph not set");
  PHMRF_CHECK(!b->ss, PHMRF_ERR_STATE, "a solve is in progress");
  PHMRF_TRY(ensure_chain_families(b));
  *n_families = (int)b->families.size();
  if (n_colours)
    for (int f = 0; f < MAX_CHAIN_FAMILIES; ++f) n_colours[f] = f < (int)b->families.size() ? b->families[f].n_colours : 0;
  return PHMRF_OK;
}

int phmrf_block_get_chain_segments(phmrf_block_t b, int family, int phase, int colour, int64_t* n_segments, int64_t* n_nodes,
                                   int32_t* seg_start, int32_t* seg_len, int32_t* nodes) {
  PHMRF_CHECK(b && n_segments && n_nodes, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(b->has_graph, PHMRF_ERR_STATE, "graph not set");
  PHMRF_CHECK(!b->ss, PHMRF_ERR_STATE, "a solve is in progress");
  PHMRF_TRY(ensure_chain_families(b));
  PHMRF_CHECK(family >= 0 && family < (int)b->families.size(), PHMRF_ERR_INVALID, "no such chain family");
  const ChainFamily& f = b->families[family];
  PHMRF_CHECK(phase == 0 || phase == 1, PHMRF_ERR_INVALID, "phase must be 0 or 1");
  PHMRF_CHECK(colour >= 0 && colour < f.n_colours, PHMRF_ERR_INVALID, "no such colour in this chain family");
  const int nseg = f.nseg[phase][colour];
  *n_segments = nseg;
  *n_nodes = f.n_nodes;
  if (seg_start && nseg > 0) PHMRF_TRY(download(seg_start, f.seg_start[phase][colour], (size_t)nseg * sizeof(int32_t), b->stream));
  if (seg_len && nseg > 0) PHMRF_TRY(download(seg_len, f.seg_len[phase][colour], (size_t)nseg * sizeof(int32_t), b->stream));
  if (nodes && f.n_nodes > 0) PHMRF_TRY(download(nodes, f.nodes, (size_t)f.n_nodes * sizeof(int32_t), b->stream));
  return PHMRF_OK;
}

int phmrf_block_prepare_components(phmrf_block_t b) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(!b->ss, PHMRF_ERR_STATE, "a solve is in progress");
  if (!b->has_labels || !b->has_graph) return PHMRF_OK;        // (nothing to prepare yet: the pass will do its own)
  return launch_component_prepare(b);
}

int phmrf_mrf_component_pass(phmrf_block_t b, double beta, int64_t* changed) {
  PHMRF_TRY(check_solvable(b));
  b->labels_are_slot = 0;
  PHMRF_TRY(zero_counter(b));
  tic(b, KC_COMPONENT);
  PHMRF_TRY(launch_component_pass(b, (float)beta));
  toc(b, KC_COMPONENT, 1);
  return read_counter(b, changed);
}

int phmrf_mrf_graph_expansion(phmrf_block_t b, double beta, int alpha, int64_t* changed) {
  PHMRF_TRY(check_solvable(b));
  PHMRF_CHECK(b->has_labels, PHMRF_ERR_STATE, "labels not set");
  PHMRF_CHECK(alpha >= 0 && alpha < b->K, PHMRF_ERR_INVALID, "alpha must be in [0, K)");
  PHMRF_CHECK(b->n >= 2, PHMRF_ERR_INVALID, "the graph has fewer than two nodes");
  b->labels_are_slot = 0;
  PHMRF_TRY(zero_counter(b));
  PHMRF_TRY(launch_graph_expansion(b, (float)beta, alpha));
  return read_counter(b, changed);
}


int phmrf_mrf_strip_pass(phmrf_block_t b, double beta, int orient, int shift_r, int shift_c, int alpha, int64_t* changed) {
  PHMRF_TRY(check_solvable(b));
  b->labels_are_slot = 0;
  PHMRF_CHECK(b->has_grid, PHMRF_ERR_STATE, "strip moves need phmrf_block_set_grid");
  PHMRF_CHECK(b->num_neighbor == 8 || b->num_neighbor == 4, PHMRF_ERR_STATE, "bad grid");
  PHMRF_CHECK(orient == 0 || orient == 1, PHMRF_ERR_INVALID, "orient must be 0 or 1");
  PHMRF_CHECK(shift_r >= 0 && shift_r <= 5 && shift_c >= 0 && shift_c <= 63, PHMRF_ERR_INVALID, "shift out of range");
  PHMRF_CHECK(alpha < b->K, PHMRF_ERR_INVALID, "alpha must be < K");
  PHMRF_TRY(zero_counter(b));
  PHMRF_TRY(strip_pass_nocount(b, (float)beta, orient, shift_r, shift_c, alpha));
  PHMRF_TRY(work_fetch_async(b));
  PHMRF_TRY(read_counter(b, changed));
  work_fold(b);
  return PHMRF_OK;
}

int phmrf_mrf_strip_multi_pass(phmrf_block_t b, double beta, int orient, int shift_r, int shift_c, uint64_t label_mask,
                               int64_t* changed) {
  PHMRF_TRY(check_solvable(b));
  b->labels_are_slot = 0;
  PHMRF_CHECK(b->has_grid, PHMRF_ERR_STATE, "strip moves need phmrf_block_set_grid");
  PHMRF_CHECK(b->num_neighbor == 8 || b->num_neighbor == 4, PHMRF_ERR_STATE, "bad grid");
  PHMRF_CHECK(orient == 0 || orient == 1, PHMRF_ERR_INVALID, "orient must be 0 or 1");
  PHMRF_CHECK(shift_r >= 0 && shift_r <= 5 && shift_c >= 0 && shift_c <= 63, PHMRF_ERR_INVALID, "shift out of range");
  PHMRF_CHECK(b->K >= 64 || (label_mask >> b->K) == 0, PHMRF_ERR_INVALID, "label_mask names a label >= K");
  PHMRF_HIP(hipMemsetAsync(b->counters, 0, N_COUNTERS * sizeof(unsigned long long), b->stream));
  if (!b->uT_valid) PHMRF_TRY(launch_unary_planes(b));
  tic(b, KC_STRIP);
  PHMRF_TRY(launch_strip_multi(b, (float)beta, orient, shift_r, shift_c, label_mask, -1));
  b->work[4] += 1;
  toc(b, KC_STRIP, 1);
  PHMRF_TRY(work_fetch_async(b));
  PHMRF_HIP(hipMemcpyAsync(b->counters_host, b->counters, N_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  work_fold(b);
  int64_t ch = 0;
  for (int a = 0; a < b->K; ++a) ch += (int64_t)b->counters_host[COUNTER_EXPANSION + a];
  if (changed) *changed = ch;
  return PHMRF_OK;
}

// ---- coarse alpha-expansions (coarse.hip; the child problems and the sweep: solve.hip) ---------------------------------
int phmrf_mrf_coarse_pass(phmrf_block_t b, double beta, int scale, int offset, int alpha, int shift_r, int shift_c,
                          int64_t* changed) {
  PHMRF_TRY(check_solvable(b));
  b->labels_are_slot = 0;
  PHMRF_CHECK(b->has_grid, PHMRF_ERR_STATE, "coarse moves need phmrf_block_set_grid");
  PHMRF_CHECK(scale == 2 || scale == 4 || scale == 8, PHMRF_ERR_INVALID, "scale must be 2, 4 or 8");
  PHMRF_CHECK(offset >= 0 && offset < scale, PHMRF_ERR_INVALID, "offset must be in [0, scale)");
  PHMRF_CHECK(alpha >= 0 && alpha < b->K, PHMRF_ERR_INVALID, "alpha must be in [0, K)");
  PHMRF_CHECK(shift_r >= 0 && shift_r <= 5 && shift_c >= 0 && shift_c <= 63, PHMRF_ERR_INVALID, "shift out of range");
  PHMRF_TRY(zero_counter(b));
  PHMRF_TRY(coarse_sweep_nocount(b, (float)beta, scale == 2 ? 0 : (scale == 4 ? 1 : 2), offset, shift_r, shift_c, alpha, alpha + 1));
  return read_counter(b, changed);
}

int phmrf_block_coarse_problem(phmrf_block_t b, double beta, int scale, int offset, int alpha, int64_t* nc, float* D_out,
                               float* lam_out) {
  PHMRF_TRY(check_solvable(b));
  PHMRF_CHECK(nc, PHMRF_ERR_INVALID, "nc is NULL");
  PHMRF_CHECK(b->has_grid, PHMRF_ERR_STATE, "coarse moves need phmrf_block_set_grid");
  PHMRF_CHECK(scale == 2 || scale == 4 || scale == 8, PHMRF_ERR_INVALID, "scale must be 2, 4 or 8");
  PHMRF_CHECK(offset >= 0 && offset < scale, PHMRF_ERR_INVALID, "offset must be in [0, scale)");
  PHMRF_CHECK(alpha >= 0 && alpha < b->K, PHMRF_ERR_INVALID, "alpha must be in [0, K)");
  *nc = coarse_nodes(b, scale, offset);
  if (!D_out && !lam_out) return PHMRF_OK;
  phmrf_block* c = nullptr;
  PHMRF_TRY(coarse_child(b, 4 * (scale == 2 ? 0 : (scale == 4 ? 1 : 2)), &c));
  if (!b->uT_valid) PHMRF_TRY(launch_unary_planes(b));
  PHMRF_TRY(launch_coarsen(b, c, scale, offset, alpha, (float)beta));
  if (D_out) PHMRF_TRY(download(D_out, c->uT + *nc, (size_t)*nc * sizeof(float), b->stream));
  if (lam_out) PHMRF_TRY(download(lam_out, c->fwd_w, (size_t)*nc * sizeof(float4), b->stream));
  return PHMRF_OK;
}

int phmrf_block_coarse_problems(phmrf_block_t b, double beta, int scale, int offset, const int* alphas, int nl, int64_t* nc,
                                float* D_out, float* lam_out) {
  PHMRF_TRY(check_solvable(b));
  PHMRF_CHECK(nc && alphas, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(b->has_grid, PHMRF_ERR_STATE, "coarse moves need phmrf_block_set_grid");
  PHMRF_CHECK(scale == 2 || scale == 4 || scale == 8, PHMRF_ERR_INVALID, "scale must be 2, 4 or 8");
  PHMRF_CHECK(offset >= 0 && offset < scale, PHMRF_ERR_INVALID, "offset must be in [0, scale)");
  PHMRF_CHECK(nl >= 1 && nl <= 4, PHMRF_ERR_INVALID, "nl must be in [1, 4]");
  for (int q = 0; q < nl; ++q) PHMRF_CHECK(alphas[q] >= 0 && alphas[q] < b->K, PHMRF_ERR_INVALID, "alpha must be in [0, K)");
  *nc = coarse_nodes(b, scale, offset);
  if (!D_out && !lam_out) return PHMRF_OK;
  const int level = scale == 2 ? 0 : (scale == 4 ? 1 : 2);
  phmrf_block* ch[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int q = 0; q < nl; ++q) PHMRF_TRY(coarse_child(b, 4 * level + q, &ch[q]));
  if (!b->uT_valid) PHMRF_TRY(launch_unary_planes(b));
  PHMRF_TRY(launch_coarsen_batch(b, ch, alphas, nl, scale, offset, (float)beta, nullptr, -1, false));
  for (int q = 0; q < nl; ++q) {
    if (D_out) PHMRF_TRY(download(D_out + (size_t)q * *nc, ch[q]->uT + *nc, (size_t)*nc * sizeof(float), b->stream));
    if (lam_out) PHMRF_TRY(download(lam_out + (size_t)q * *nc * 4, ch[q]->fwd_w, (size_t)*nc * sizeof(float4), b->stream));
  }
  return PHMRF_OK;
}

int phmrf_mrf_coarse_sweep(phmrf_block_t b, double beta, int scale, int offset, uint64_t label_mask, int shift_r, int shift_c,
                           int stamps, int64_t* changed, int64_t* changed_label) {
  PHMRF_TRY(check_solvable(b));
  PHMRF_CHECK(!b->ss, PHMRF_ERR_STATE, "a solve is in progress");
  PHMRF_CHECK(b->has_grid, PHMRF_ERR_STATE, "coarse moves need phmrf_block_set_grid");
  PHMRF_CHECK(b->has_labels, PHMRF_ERR_STATE, "labels not set");
  PHMRF_CHECK(scale == 2 || scale == 4 || scale == 8, PHMRF_ERR_INVALID, "scale must be 2, 4 or 8");
  PHMRF_CHECK(offset >= 0 && offset < scale, PHMRF_ERR_INVALID, "offset must be in [0, scale)");
  PHMRF_CHECK(shift_r >= 0 && shift_r <= 5 && shift_c >= 0 && shift_c <= 63, PHMRF_ERR_INVALID, "shift out of range");
  PHMRF_CHECK(b->K >= 64 || (label_mask >> b->K) == 0, PHMRF_ERR_INVALID, "label_mask names a label >= K");
  b->labels_are_slot = 0;
  const int level = scale == 2 ? 0 : (scale == 4 ? 1 : 2);
  const size_t lab_bytes = (size_t)N_COARSE * MAX_LABELS * sizeof(unsigned long long);
  if (!b->coarse_lab) {
    PHMRF_TRY(dev_alloc(&b->coarse_lab, (size_t)N_COARSE * MAX_LABELS));
    PHMRF_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->coarse_lab_host), lab_bytes));
  }
  PHMRF_HIP(hipMemsetAsync(b->coarse_lab, 0, lab_bytes, b->stream));
  PHMRF_TRY(zero_counter(b));
  if (stamps) {         // as solve_begin leaves them: no node stamped, the first launch tick
    if (!b->stamp) PHMRF_TRY(dev_alloc(&b->stamp, (size_t)b->n));
    PHMRF_HIP(hipMemsetAsync(b->stamp, 0, (size_t)b->n * sizeof(uint16_t), b->stream));
    b->tick = 1;
  }
  int st = coarse_sweep_nocount(b, (float)beta, level, offset, shift_r, shift_c, 0, b->K, label_mask);
  if (st == PHMRF_OK && hipMemcpyAsync(b->coarse_lab_host, b->coarse_lab, lab_bytes, hipMemcpyDeviceToHost, b->stream) != hipSuccess)
    st = PHMRF_ERR_HIP;
  const int st_read = read_counter(b, changed);
  if (stamps) solve_scope_exit(b);
  PHMRF_TRY(st);
  PHMRF_TRY(st_read);
  if (changed_label)
    for (int a = 0; a < b->K; ++a) changed_label[a] = (int64_t)b->coarse_lab_host[(size_t)level * MAX_LABELS + a];
  return PHMRF_OK;
}

// ---- the coarse-to-fine start's child problem (c2f.hip; built by solve.hip) ----------------------------------------------
static int c2f_ready(phmrf_block_t b) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(!b->ss, PHMRF_ERR_STATE, "a solve is in progress");
  PHMRF_CHECK(c2f_applies(b), PHMRF_ERR_STATE,
              "the coarse-to-fine start needs a complete 8-neighbour grid block (no row tile) with n >= 1024 and H, W >= 8");
  return c2f_child(b);
}

int phmrf_block_c2f_problem(phmrf_block_t b, int* Hc, int* Wc, int64_t* nc, int32_t* nbr_out, float* wgt_out, float* logprob_out) {
  PHMRF_TRY(check_solvable(b));
  PHMRF_CHECK(Hc && Wc && nc, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_TRY(c2f_ready(b));
  phmrf_block* c = b->c2f;
  *Hc = b->c2f_Hc;
  *Wc = b->c2f_Wc;
  *nc = c->n;
  if (nbr_out) PHMRF_TRY(download(nbr_out, c->nbr, (size_t)c->n * 8 * sizeof(int32_t), b->stream));
  if (wgt_out) PHMRF_TRY(download(wgt_out, c->wgt, (size_t)c->n * 8 * sizeof(float), b->stream));
  if (logprob_out) {
    PHMRF_TRY(launch_c2f_logprob(b, c, b->c2f_Wc, C2F_SCALE));
    c->has_logprob = true;
    c->uT_valid = false;
    PHMRF_TRY(download(logprob_out, c->logprob, (size_t)c->n * b->K * sizeof(float), b->stream));
  }
  return PHMRF_OK;
}

int phmrf_block_c2f_prolong(phmrf_block_t b, const int32_t* labels_c, int64_t nc) {
  PHMRF_CHECK(b && labels_c, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_TRY(c2f_ready(b));
  phmrf_block* c = b->c2f;
  PHMRF_CHECK(nc == c->n, PHMRF_ERR_INVALID, "nc is not the number of 4 x 4 super-cells");
  std::vector<uint8_t> tmp((size_t)nc);
  for (int64_t i = 0; i < nc; ++i) {
    PHMRF_CHECK(labels_c[i] >= 0 && labels_c[i] < b->K, PHMRF_ERR_INVALID, "label out of range [0,K)");
    tmp[(size_t)i] = (uint8_t)labels_c[i];
  }
  PHMRF_TRY(upload(c->labels, tmp.data(), (size_t)nc, b->stream));
  c->has_labels = true;
  c->labels_are_slot = 0;
  PHMRF_TRY(launch_c2f_prolong(b, c, b->c2f_Wc, C2F_SCALE));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  b->has_labels = true;
  b->labels_are_slot = 0;
  return PHMRF_OK;
}

// ---- row tiles (tile.hip) -----------------------------------------------------------------------

int phmrf_block_set_tile(phmrf_block_t b, int top, int bottom, int64_t sched_n) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(b->has_grid, PHMRF_ERR_STATE, "row tiles need the grid geometry (phmrf_block_set_grid / build_grid_graph)");
  PHMRF_CHECK(!b->ss, PHMRF_ERR_STATE, "a solve is in progress");
  top = top ? 1 : 0;
  bottom = bottom ? 1 : 0;
  PHMRF_CHECK(b->H >= 2 * (top + bottom) + 2, PHMRF_ERR_INVALID, "a tile needs two rows per cut and two more");
  for (int r = 0; r < 2; ++r) {
    dev_free(b->pin_save[r]);
    dev_free(b->pin_label[r]);
    b->pin_first[r] = b->pin_count[r] = b->pin_split[r] = 0;
    b->pin_rows[r] = 0;
  }
  b->pin_saved = false;
  b->tile_top = top;
  b->tile_bot = bottom;
  b->sched_n = sched_n > 0 ? sched_n : 0;
  if (!top && !bottom) {
    b->own0 = 0;
    b->own1 = -1;
    b->own_r0 = 0;
    b->own_r1 = -1;
    return PHMRF_OK;
  }
  b->own_r0 = top ? 1 : 0;
  b->own_r1 = b->H - (bottom ? 1 : 0);
  b->own0 = row_first(b, b->own_r0);
  b->own1 = row_first(b, b->own_r1);
  if (top) {
    b->pin_first[0] = 0;
    b->pin_count[0] = row_first(b, 2);
    b->pin_split[0] = row_first(b, 1);
  }
  if (bottom) {
    b->pin_first[1] = row_first(b, b->H - 2);
    b->pin_count[1] = b->n - b->pin_first[1];
    b->pin_split[1] = row_first(b, b->H - 1) - b->pin_first[1];
  }
  int64_t cap = 0;
  for (int r = 0; r < 2; ++r)
    if (b->pin_count[r] > 0) {
      PHMRF_TRY(dev_alloc(&b->pin_save[r], (size_t)b->pin_count[r] * b->K));
      PHMRF_TRY(dev_alloc(&b->pin_label[r], (size_t)b->pin_count[r]));
      cap += b->pin_count[r];
    }
  if (cap > b->xfer_cap) {
    dev_free(b->xfer);
    if (b->xfer_host) (void)hipHostFree(b->xfer_host);
    b->xfer_host = nullptr;
    PHMRF_TRY(dev_alloc(&b->xfer, (size_t)cap));
    PHMRF_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->xfer_host), (size_t)2 * cap));     // outgoing | incoming rows
    b->xfer_cap = cap;
  }
  return PHMRF_OK;
}

// the node range of the first (from the top) / last (from the bottom) `rows` rows of a pin region
static void pin_range(const phmrf_block* b, int region, int rows, int64_t* first, int64_t* count) {
  *first = b->pin_first[region];
  *count = 0;
  if (rows <= 0 || b->pin_count[region] == 0) return;
  if (rows >= 2) {
    *count = b->pin_count[region];
  } else if (region == 0) {
    *count = b->pin_split[0];
  } else {
    *first = b->pin_first[1] + b->pin_split[1];
    *count = b->pin_count[1] - b->pin_split[1];
  }
}

int phmrf_block_tile_pins(phmrf_block_t b, int n_top, int n_bottom) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(is_tile(b), PHMRF_ERR_STATE, "the block is not a tile (phmrf_block_set_tile)");
  PHMRF_CHECK(b->has_logprob, PHMRF_ERR_STATE, "logprob not set");
  PHMRF_CHECK(n_top >= 0 && n_top <= 2 && n_bottom >= 0 && n_bottom <= 2, PHMRF_ERR_INVALID, "0, 1 or 2 rows per cut");
  const int want[2] = {b->tile_top ? n_top : 0, b->tile_bot ? n_bottom : 0};
  if (b->tick) ++b->tick;                  // (one tick whatever the tile's cuts: the tiles of a block count alike)
  for (int r = 0; r < 2; ++r) {
    if (b->pin_count[r] == 0) continue;
    int64_t pf, pc, wf, wc;
    pin_range(b, r, want[r], &pf, &pc);
    pin_range(b, r, b->pin_saved ? b->pin_rows[r] : 0, &wf, &wc);
    PHMRF_TRY(launch_tile_pins(b, r, b->pin_first[r], b->pin_count[r], pf, pc, wf, wc, !b->pin_saved));
    b->pin_rows[r] = want[r];
  }
  b->pin_saved = true;
  return PHMRF_OK;
}

// the rows the neighbour tiles need: top_out = the first row this tile owns, bottom_out = the last (either may be NULL)
int phmrf_block_tile_get_boundary(phmrf_block_t b, uint8_t* top_out, uint8_t* bottom_out) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(is_tile(b), PHMRF_ERR_STATE, "the block is not a tile (phmrf_block_set_tile)");
  // inside a solve the rows were queued behind the round's moves (solve_round_launch) and have arrived with the round's
  // counters (solve_round_collect): no device traffic, no wait
  const bool have = b->boundary_queued && b->ss && b->ss->collected;
  if (!have) {
    PHMRF_TRY(tile_queue_boundary(b));
    PHMRF_HIP(hipStreamSynchronize(b->stream));
  }
  b->boundary_queued = false;
  int64_t off = 0;
  if (b->tile_top) {
    const int64_t tc = row_first(b, 2) - row_first(b, 1);
    if (top_out) std::memcpy(top_out, b->xfer_host, (size_t)tc);
    off = tc;
  }
  if (b->tile_bot && bottom_out) {
    const int64_t bc = row_first(b, b->H - 1) - row_first(b, b->H - 2);
    std::memcpy(bottom_out, b->xfer_host + off, (size_t)bc);
  }
  return PHMRF_OK;
}

// the neighbours' rows: top_in -> this tile's first row (its upper halo), bottom_in -> its last row (either may be NULL)
int phmrf_block_tile_put_halo(phmrf_block_t b, const uint8_t* top_in, const uint8_t* bottom_in) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(is_tile(b), PHMRF_ERR_STATE, "the block is not a tile (phmrf_block_set_tile)");
  if (b->tick) ++b->tick;
  b->labels_are_slot = 0;
  uint8_t* const in_host = b->xfer_host + b->xfer_cap;      // (the second half of the pinned buffer: the first holds the outgoing rows)
  int64_t off = 0;
  if (top_in && b->tile_top) {
    const int64_t c = row_first(b, 1);
    for (int64_t q = 0; q < c; ++q) PHMRF_CHECK(top_in[q] < b->K, PHMRF_ERR_INVALID, "label out of range [0,K)");
    std::memcpy(in_host, top_in, (size_t)c);
    PHMRF_HIP(hipMemcpyAsync(b->xfer, in_host, (size_t)c, hipMemcpyHostToDevice, b->stream));
    PHMRF_TRY(launch_put_labels(b, 0, c, b->xfer));
    off = c;
  }
  if (bottom_in && b->tile_bot) {
    const int64_t f = row_first(b, b->H - 1), c = b->n - f;
    for (int64_t q = 0; q < c; ++q) PHMRF_CHECK(bottom_in[q] < b->K, PHMRF_ERR_INVALID, "label out of range [0,K)");
    std::memcpy(in_host + off, bottom_in, (size_t)c);
    PHMRF_HIP(hipMemcpyAsync(b->xfer + off, in_host + off, (size_t)c, hipMemcpyHostToDevice, b->stream));
    PHMRF_TRY(launch_put_labels(b, f, c, b->xfer + off));
  }
  // (no wait: inside a solve the next call comes after the next round has been collected -- a stream synchronisation --,
  //  so the copies have left the staging buffers by then; outside a solve the caller's next synchronising call does it)
  if (!b->ss) PHMRF_HIP(hipStreamSynchronize(b->stream));
  return PHMRF_OK;
}

// ---- b3 posterior / stats -----------------------------------------------------------------------
static int posterior_launch(phmrf_block_t b, double beta, int estimate_type, bool write_post) {
  PHMRF_TRY(check_solvable(b));
  PHMRF_CHECK(b->has_X, PHMRF_ERR_STATE, "observations not set");
  const int ns = n_stats(b);
  PHMRF_CHECK(8 + ns <= ACCUM_DOUBLES, PHMRF_ERR_UNSUPPORTED, "K*(1+S+S*S) too large");
  if (write_post && !b->posteriors) PHMRF_TRY(dev_alloc(&b->posteriors, (size_t)b->n * b->K));
  if (b->deterministic && !b->post_partial) {       // one row per workgroup of the kernel's grid over at most n nodes
    const int64_t rows = std::min<int64_t>(POST_PARTIAL_ROWS, std::max<int64_t>(1, (b->n + POST_DET_TB - 1) / POST_DET_TB));
    PHMRF_TRY(dev_alloc(&b->post_partial, (size_t)rows * (b->K * (1 + b->S + b->S * (b->S + 1) / 2) + 4)));   // 1 | x | x_s x_t
  }
  PHMRF_TRY(zero_accum(b, 0, 4));
  PHMRF_TRY(zero_accum(b, 8, ns));
  tic(b, KC_POSTERIOR);
  PHMRF_TRY(launch_posterior_stats(b, (float)beta, estimate_type, write_post));
  toc(b, KC_POSTERIOR, 1);
  return PHMRF_OK;
}

int phmrf_posterior_stats(phmrf_block_t b, double beta, int estimate_type, double* stats_out, double* costs_out,
                          double* posteriors_out) {
  PHMRF_CHECK(b && stats_out && costs_out, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_TRY(posterior_launch(b, beta, estimate_type, posteriors_out != nullptr));
  const int ns = n_stats(b);
  PHMRF_HIP(hipMemcpyAsync(b->accum_host, b->accum, (8 + ns) * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  std::memcpy(costs_out, b->accum_host, 4 * sizeof(double));
  std::memcpy(stats_out, b->accum_host + 8, ns * sizeof(double));
  if (posteriors_out) {
    const size_t cnt = (size_t)b->n * b->K;
    std::vector<float> tmp(cnt);
    PHMRF_TRY(download(tmp.data(), b->posteriors, cnt * sizeof(float), b->stream));
    for (size_t i = 0; i < cnt; ++i) posteriors_out[i] = tmp[i];
  }
  return PHMRF_OK;
}

int phmrf_posterior_stats_dev(phmrf_block_t b, double beta, int estimate_type, double* out_dev) {
  PHMRF_CHECK(b && out_dev, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_TRY(posterior_launch(b, beta, estimate_type, false));
  const int ns = n_stats(b);
  PHMRF_HIP(hipMemcpyAsync(out_dev, b->accum + 8, ns * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
  PHMRF_HIP(hipMemcpyAsync(out_dev + ns, b->accum, 4 * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
  return PHMRF_OK;
}

// per-node summary of the posteriors of the owned rows (no statistics): three device arrays, then one download each
int phmrf_posterior_summary(phmrf_block_t b, double beta, int estimate_type, float* conf, uint8_t* top, float* entropy_or_null) {
  PHMRF_CHECK(b && conf && top, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_TRY(check_solvable(b));
  PHMRF_CHECK(b->has_labels, PHMRF_ERR_STATE, "labels not set (phmrf_block_set_labels or a solve)");
  const int64_t n_first = b->own1 >= 0 ? b->own0 : 0, n_last = b->own1 >= 0 ? b->own1 : b->n;
  const int64_t m = n_last - n_first;
  if (m <= 0) return PHMRF_OK;
  if (!b->summary) PHMRF_TRY(dev_alloc(&b->summary, (size_t)b->n * (2 * sizeof(float) + 1)));
  float* d_conf = reinterpret_cast<float*>(b->summary);
  float* d_ent = d_conf + b->n;
  uint8_t* d_top = reinterpret_cast<uint8_t*>(d_ent + b->n);
  tic(b, KC_POSTERIOR);
  PHMRF_TRY(launch_posterior_summary(b, (float)beta, estimate_type, d_conf, d_top, entropy_or_null ? d_ent : nullptr));
  toc(b, KC_POSTERIOR, 1);
  PHMRF_HIP(hipMemcpyAsync(conf, d_conf, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipMemcpyAsync(top, d_top, (size_t)m, hipMemcpyDeviceToHost, b->stream));
  if (entropy_or_null)
    PHMRF_HIP(hipMemcpyAsync(entropy_or_null, d_ent, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  return PHMRF_OK;
}

// posterior-weighted (weighting 0) or called-state (1) affine maps of the observations over the owned rows: the tables go
// to the device as f32 [K][A][S+2] = c | g | v, the planes come back with one download each
int phmrf_ancestral(phmrf_block_t b, double beta, int estimate_type, int weighting, int A, const double* affine,
                    const double* cond_var, float* mean_out, float* sd_out_or_null) {
  PHMRF_CHECK(b && affine && cond_var && mean_out, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(weighting == 0 || weighting == 1, PHMRF_ERR_INVALID, "weighting must be 0 (posterior) or 1 (called)");
  PHMRF_CHECK(A >= 1 && A <= 16, PHMRF_ERR_UNSUPPORTED, "ancestral: A must be in [1,16]");
  PHMRF_CHECK(b->S <= 8, PHMRF_ERR_UNSUPPORTED, "ancestral: S must be in [1,8]");
  const int K = b->K, S = b->S, TS = S + 2;
  std::vector<float> tab((size_t)K * A * TS);
  for (int ka = 0; ka < K * A; ++ka) {
    for (int s = 0; s <= S; ++s) tab[(size_t)ka * TS + s] = (float)affine[(size_t)ka * (S + 1) + s];
    tab[(size_t)ka * TS + S + 1] = (float)cond_var[ka];
    PHMRF_CHECK(cond_var[ka] >= 0.0, PHMRF_ERR_INVALID, "cond_var must be finite and >= 0");
  }
  for (float v : tab) PHMRF_CHECK(std::isfinite(v), PHMRF_ERR_INVALID, "the tables must be finite (as float32)");
  PHMRF_CHECK(b->has_X, PHMRF_ERR_STATE, "observations not set");
  PHMRF_CHECK(b->has_labels, PHMRF_ERR_STATE, "labels not set (phmrf_block_set_labels or a solve)");
  if (weighting == 0) PHMRF_TRY(check_solvable(b));
  const int64_t n_first = b->own1 >= 0 ? b->own0 : 0, n_last = b->own1 >= 0 ? b->own1 : b->n;
  const int64_t m = n_last - n_first;
  if (m <= 0) return PHMRF_OK;
  const size_t need = tab.size() + (size_t)2 * A * m;
  if (b->anc_floats < need) {
    dev_free(b->anc);
    b->anc_floats = 0;
    PHMRF_TRY(dev_alloc(&b->anc, need));
    b->anc_floats = need;
  }
  float* d_mean = b->anc + tab.size();
  float* d_sd = d_mean + (size_t)A * m;
  PHMRF_TRY(upload(b->anc, tab.data(), tab.size() * sizeof(float), b->stream));
  tic(b, KC_POSTERIOR);
  PHMRF_TRY(launch_ancestral(b, (float)beta, estimate_type, weighting, A, b->anc, d_mean, sd_out_or_null ? d_sd : nullptr));
  toc(b, KC_POSTERIOR, 1);
  PHMRF_HIP(hipMemcpyAsync(mean_out, d_mean, (size_t)A * m * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  if (sd_out_or_null)
    PHMRF_HIP(hipMemcpyAsync(sd_out_or_null, d_sd, (size_t)A * m * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  return PHMRF_OK;
}

// ---- initialisation -----------------------------------------------------------------------------
int phmrf_kmeans_step(phmrf_block_t b, const double* centers, int write_labels, double* out) {
  PHMRF_CHECK(b && centers && out, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(b->has_X, PHMRF_ERR_STATE, "observations not set");
  const int K = b->K, S = b->S, NP = K * S + K + 1;
  PHMRF_CHECK(8 + NP <= ACCUM_DOUBLES, PHMRF_ERR_UNSUPPORTED, "K*S too large");
  std::vector<float> c((size_t)K * S);
  for (int i = 0; i < K * S; ++i) {
    PHMRF_CHECK(std::isfinite(centers[i]), PHMRF_ERR_INVALID, "centres must be finite");
    c[i] = (float)centers[i];
  }
  PHMRF_TRY(upload(b->emis_params, c.data(), c.size() * sizeof(float), b->stream));   // K*S floats fit the emission pack
  PHMRF_TRY(zero_accum(b, 8, NP));
  PHMRF_TRY(launch_kmeans_step(b, b->emis_params, write_labels != 0, b->accum + 8));
  PHMRF_HIP(hipMemcpyAsync(b->accum_host + 8, b->accum + 8, NP * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  std::memcpy(out, b->accum_host + 8, NP * sizeof(double));
  if (write_labels) {
    b->has_labels = true;
    b->labels_are_slot = 0;
  }
  return PHMRF_OK;
}

int phmrf_kmeans_moments(phmrf_block_t b, const double* centers, int write_labels, double* out) {
  PHMRF_CHECK(b && centers && out, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(b->has_X, PHMRF_ERR_STATE, "observations not set");
  const int K = b->K, S = b->S, NP = K * S + K + 1 + K * S * S;
  PHMRF_CHECK(S <= 8, PHMRF_ERR_UNSUPPORTED, "second moments: S must be in [1,8]");
  PHMRF_CHECK(8 + NP <= ACCUM_DOUBLES, PHMRF_ERR_UNSUPPORTED, "K*S*S too large");
  std::vector<float> c((size_t)K * S);
  for (int i = 0; i < K * S; ++i) {
    PHMRF_CHECK(std::isfinite(centers[i]), PHMRF_ERR_INVALID, "centres must be finite");
    c[i] = (float)centers[i];
  }
  PHMRF_TRY(upload(b->emis_params, c.data(), c.size() * sizeof(float), b->stream));
  PHMRF_TRY(zero_accum(b, 8, NP));
  PHMRF_TRY(launch_kmeans_step(b, b->emis_params, write_labels != 0, b->accum + 8, true));
  PHMRF_HIP(hipMemcpyAsync(b->accum_host + 8, b->accum + 8, NP * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  std::memcpy(out, b->accum_host + 8, NP * sizeof(double));
  if (write_labels) {
    b->has_labels = true;
    b->labels_are_slot = 0;
  }
  return PHMRF_OK;
}

// ---- measurement --------------------------------------------------------------------------------
int phmrf_block_enable_timing(phmrf_block_t b, int enable) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  b->timing = enable != 0;
  return PHMRF_OK;
}

int phmrf_block_set_timing_classes(phmrf_block_t b, uint32_t class_mask) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  b->timing_mask = class_mask;
  return PHMRF_OK;
}

static int get_timing(phmrf_block_t b, bool first, int capacity, double* ms, int64_t* launches) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  PHMRF_CHECK(capacity >= 0, PHMRF_ERR_INVALID, "capacity < 0");
  resolve_timing(b);
  for (int i = 0; i < PHMRF_NUM_KERNEL_CLASSES && i < capacity; ++i) {
    if (ms) ms[i] = first ? b->ms_first[i] : b->ms[i];
    if (launches) launches[i] = first ? b->launches_first[i] : b->launches[i];
  }
  return PHMRF_OK;
}
int phmrf_block_get_timing(phmrf_block_t b, int capacity, double* ms, int64_t* launches) { return get_timing(b, false, capacity, ms, launches); }
int phmrf_block_get_timing_first(phmrf_block_t b, int capacity, double* ms, int64_t* launches) { return get_timing(b, true, capacity, ms, launches); }

int phmrf_block_reset_timing(phmrf_block_t b) {
  PHMRF_CHECK(b, PHMRF_ERR_INVALID, "block is NULL");
  resolve_timing(b);
  for (int i = 0; i < PHMRF_NUM_KERNEL_CLASSES; ++i) {
    b->ms[i] = b->ms_first[i] = 0;
    b->launches[i] = b->launches_first[i] = 0;
  }
  for (int q = 0; q < N_WORK; ++q) b->work[q] = b->work_first[q] = 0;
  PHMRF_HIP(hipMemsetAsync(b->work_acc, 0, WORK_BANKS * WORK_SLOTS * sizeof(unsigned long long), b->stream));
  b->intervals.clear();
  return PHMRF_OK;
}

int phmrf_time_base_reset(void) {
  int dev = 0;
  PHMRF_HIP(hipGetDevice(&dev));
  PHMRF_CHECK(dev >= 0 && dev < 64, PHMRF_ERR_UNSUPPORTED, "device index >= 64");
  if (!g_time_base[dev]) PHMRF_HIP(hipEventCreate(&g_time_base[dev]));
  PHMRF_HIP(hipDeviceSynchronize());
  PHMRF_HIP(hipEventRecord(g_time_base[dev], nullptr));
  PHMRF_HIP(hipEventSynchronize(g_time_base[dev]));
  return PHMRF_OK;
}

int phmrf_block_get_work(phmrf_block_t b, int64_t* out) {
  PHMRF_CHECK(b && out, PHMRF_ERR_INVALID, "NULL argument");
  for (int q = 0; q < 8; ++q) out[q] = b->work[q];
  return PHMRF_OK;
}

int phmrf_block_get_work_first(phmrf_block_t b, int64_t* out) {
  PHMRF_CHECK(b && out, PHMRF_ERR_INVALID, "NULL argument");
  for (int q = 0; q < 8; ++q) out[q] = b->work_first[q];
  return PHMRF_OK;
}

int phmrf_block_get_work_ex(phmrf_block_t b, int first_round_only, int capacity, int64_t* out) {
  PHMRF_CHECK(b && out, PHMRF_ERR_INVALID, "NULL argument");
  for (int q = 0; q < N_WORK && q < capacity; ++q) out[q] = first_round_only ? b->work_first[q] : b->work[q];
  return PHMRF_OK;
}

int phmrf_block_get_intervals(phmrf_block_t b, int kclass, double* out, int64_t capacity, int64_t* count) {
  PHMRF_CHECK(b && count, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(kclass >= 0 && kclass < PHMRF_NUM_KERNEL_CLASSES, PHMRF_ERR_INVALID, "no such kernel class");
  resolve_timing(b);
  int64_t c = 0;
  for (const auto& iv : b->intervals)
    if (iv.kclass == kclass) {
      if (out && c < capacity) {
        out[2 * c] = iv.t0;
        out[2 * c + 1] = iv.t1;
      }
      ++c;
    }
  *count = c;
  return PHMRF_OK;
}

}  // extern "C"
