// gfx950 kernels of the rescaled pile-up of ONE chromosome's state map over features of unequal size (phmrf_state_aggregate;
// DESIGN.md section 7).  A feature is two bin intervals A and B with a group and a flip; each axis is cut into P = T + 2 F
// cells, edge(c) = x0 + floor((c - F) n / T), cell c = [edge(c), max(edge(c) + 1, edge(c + 1))), and pile cell (u, v) is the
// rectangle I x J of cell u of A and cell v of B (both indices reversed when flipped).  hist[f][u][v][k] = over the stored
// nodes (p, q) of EVERY region in state k: [(p, q) in I x J] + [p != q and (q, p) in I x J];
//   cells[g][u][v][k] = the sum of hist over the features of group g, votes[g][u][v][k] = the features of group g whose
//   hist[f][u][v] is not empty and has its maximum at k, the lowest k on ties.
// Integer arithmetic throughout, no floating point: no result depends on the order in which the atomics land.
//
//   The axis map without a division per cell: n = qn T + rn once per feature, then (c - F) n / T = (c - F) qn + (c - F) rn / T
//   and the second term's numerator is a small int, -32 * 63 .. 96 * 63.  Its true floor is ((x + 32 T) M >> 24) - 32 with
//   M = ceil(2^24 / T): x + 32 T is in [0, 128 T), the error of M T against 2^24 is below T <= 64, and 128 * 64 * 64 < 2^24,
//   so the shift is the exact quotient; the product stays below 2^32.  The first term and the edge are 64-bit.
//
//   A feature is SMALL when ceil(nA / T) ceil(nB / T) <= AGG_SMALL_AREA bin pairs (no cell of it is larger), else LARGE; the
//   two kinds go through two kernels, each of which passes over the other's features after one uniform load.
//   aggregate_lane_kernel (small): pileup.hip's decomposition.  An item is a tile of AGG_LANES consecutive pile cells times a
//   chunk of at most AGG_CHUNK consecutive features of one group; lane <-> pile cell.  The lane walks its cell's rectangle
//   in both orientations through every region the feature's window touches (the region loop is uniform over the workgroup)
//   into a PRIVATE column of 16-bit counters in LDS, [k / 2][lane]: a rectangle clipped to a region holds at most
//   AGG_SMALL_AREA nodes, so 2 * 256 * 64 regions = 32,768 is the most a counter sees.  After the feature the lane reads its
//   column once: the arg-max becomes one vote in a second 16-bit column (a chunk has at most 256 features), the counts go
//   to a third column of u32 (256 * 32,768 = 2^23), the first is zeroed.  No LDS atomics, no bank conflicts (a lane's words
//   fall on bank lane mod 32 of its half-wave), no barrier.  After the chunk the non-zero entries go out with u64 atomics.
//   At K = 64 the three columns take 64 KB.
//   aggregate_wave_kernel (large): an item is (feature, pile row u); the four waves of a workgroup take the cells v of the
//   row in turn and share nothing.  A wave walks every clipped rectangle row by row in pieces of at most 256 columns through
//   label_row / wave_run_add (runs.h) into a private u32 histogram in LDS, as rect_states_kernel does; after each rectangle
//   (fewer than 2^31 nodes: no carry) lane k moves bin k into a 64-bit register.  One wave reduction gives the arg-max;
//   the non-zero totals and the vote go out with u64 atomics.
//   A feature whose window misses every region, and a cell whose rectangle misses a region, cost no label load.
//   Flag bits: a label >= K inside a cell, a flip > 1, a coordinate with |c| >= 2^30, an empty interval.

#include "interval_lists.h"

namespace phmrf {
namespace {

constexpr int AGG_LANES = 128;           // pile cells of a tile = lanes of a workgroup of the lane kernel (aggregate.py LANES)
constexpr int AGG_CHUNK = 256;           // features of one group a workgroup piles before it adds to the tables (aggregate.py CHUNK)
constexpr int AGG_GRID_CAP = 4096;       // workgroups of the lane kernel (aggregate.py GRID_CAP)
constexpr int AGG_SMALL_AREA = 256;      // a feature with ceil(nA / T) ceil(nB / T) above this goes a wave per cell (aggregate.py SMALL_AREA)
constexpr int AGG_WAVES = 4;             // waves of a workgroup of the wave kernel (aggregate.py WAVES)
constexpr int AGG_WAVE_GRID_CAP = 2048;  // workgroups of the wave kernel (aggregate.py WAVE_GRID_CAP)
constexpr int AGG_ROW_W = 256;           // columns of a row piece: at most one 4-byte word a lane
constexpr int AGG_MAX_BODY = 64;         // T <= 64 (aggregate.py MAX_BODY)
constexpr int AGG_MAX_FLANK = 32;        // F <= 32 (aggregate.py MAX_FLANK)
constexpr int AGG_MAX_REGIONS = 64;      // R <= 64: a feature's regions are a 64-bit mask (aggregate.py MAX_REGIONS)
constexpr int64_t AGG_MAX_TABLE = (int64_t)1 << 24;      // G P P K entries of either table (aggregate.py MAX_TABLE)
constexpr int BAD_LABEL = 1, BAD_FLIP = 2, BAD_COORD = 4, BAD_EMPTY = 8;

static_assert(2 * AGG_SMALL_AREA * AGG_MAX_REGIONS < 65536, "a 16-bit counter holds a small cell's histogram");
static_assert(AGG_CHUNK < 65536, "a 16-bit counter holds a chunk's votes");
static_assert((int64_t)AGG_CHUNK * 2 * AGG_SMALL_AREA * AGG_MAX_REGIONS < ((int64_t)1 << 32), "a u32 holds a chunk's counts");
static_assert(AGG_ROW_W == 4 * 64, "a row piece is at most one word per lane");
static_assert(128 * AGG_MAX_BODY * AGG_MAX_BODY < (1 << 24), "the multiply-shift of agg_edge is the exact quotient");

// a region of the chromosome: its slice of the labels starts at lo
struct AggRegion {
  long long lo;
  int H, W, s1, s2, diagonal, pad;
};

struct AggGrid {
  int T, F, P, magic;                    // magic = ceil(2^24 / T)
};

struct AggAxis {
  long long x0, qn;                      // the interval starts at x0 and has qn T + rn bins
  int rn;
};

// one checked feature: A and B, reversed or not, and the regions its window may touch
struct AggFeature {
  AggAxis A, B;
  int flip;
  bool small;
  unsigned long long mask;
};

inline size_t aggregate_lds_bytes(int K) { return (size_t)4 * ((K + 1) / 2) * AGG_LANES * sizeof(unsigned); }

__device__ __forceinline__ long long agg_edge(const AggAxis& a, int c, const AggGrid& gd) {
  const int d = c - gd.F;
  const int frac = (int)(((unsigned)(d * a.rn + AGG_MAX_FLANK * gd.T) * (unsigned)gd.magic) >> 24) - AGG_MAX_FLANK;
  return a.x0 + (long long)d * a.qn + frac;
}

// cell c of the axis: [*lo, *hi)
__device__ __forceinline__ void agg_cell(const AggAxis& a, int c, const AggGrid& gd, long long* lo, long long* hi) {
  *lo = agg_edge(a, c, gd);
  const long long e = agg_edge(a, c + 1, gd);
  *hi = e > *lo ? e : *lo + 1;
}

__device__ __forceinline__ bool agg_meets(long long lo, long long hi, int start, int n) { return lo < (long long)start + n && hi > start; }

// feature f (the same for every lane); false: it is passed over, with a flag bit in *wrong when it is malformed
__device__ __forceinline__ bool agg_feature(const int32_t* __restrict__ feat, const uint8_t* __restrict__ flip, int64_t f,
                                            const AggGrid& gd, const AggRegion* __restrict__ regs, int R, AggFeature* ft, int* wrong) {
  const int a0 = feat[4 * f], a1 = feat[4 * f + 1], b0 = feat[4 * f + 2], b1 = feat[4 * f + 3];
  ft->flip = flip ? flip[f] : 0;
  int w = 0;
  if (ft->flip > 1) w |= BAD_FLIP;
  if (coord_out(a0) || coord_out(a1) || coord_out(b0) || coord_out(b1))
    w |= BAD_COORD;
  else if (a1 <= a0 || b1 <= b0)
    w |= BAD_EMPTY;
  if (w) {
    *wrong |= w;
    return false;
  }
  const unsigned na = (unsigned)(a1 - a0), nb = (unsigned)(b1 - b0), T = (unsigned)gd.T;       // below 2^31
  ft->A.x0 = a0;
  ft->A.qn = na / T;
  ft->A.rn = (int)(na - (unsigned)ft->A.qn * T);
  ft->B.x0 = b0;
  ft->B.qn = nb / T;
  ft->B.rn = (int)(nb - (unsigned)ft->B.qn * T);
  const long long wa = ft->A.qn + (ft->A.rn ? 1 : 0), wb = ft->B.qn + (ft->B.rn ? 1 : 0);      // >= 1 each
  ft->small = wa * wb <= AGG_SMALL_AREA;
  // the window of an axis: every cell lies in [edge(0), edge(P) + 1)
  const long long al = agg_edge(ft->A, 0, gd), ah = agg_edge(ft->A, gd.P, gd) + 1;
  const long long bl = agg_edge(ft->B, 0, gd), bh = agg_edge(ft->B, gd.P, gd) + 1;
  unsigned long long mask = 0;
  for (int r = 0; r < R; ++r) {
    const AggRegion rg = regs[r];
    if ((agg_meets(al, ah, rg.s1, rg.H) && agg_meets(bl, bh, rg.s2, rg.W)) ||
        (agg_meets(bl, bh, rg.s1, rg.H) && agg_meets(al, ah, rg.s2, rg.W)))
      mask |= 1ull << r;
  }
  ft->mask = mask;
  return mask != 0;
}

// rows [rlo, rhi) and columns [clo, chi) in chromosome bins -> local to the region and clipped; false: nothing stored there
__device__ __forceinline__ bool agg_clip(const AggRegion& rg, long long rlo, long long rhi, long long clo, long long chi, int* i0,
                                         int* i1, int* j0, int* j1) {
  return clip_rect(rg.H, rg.W, rg.diagonal, rlo - rg.s1, rhi - rg.s1, clo - rg.s2, chi - rg.s2, i0, i1, j0, j1);
}

// cells, votes: u64 [G][P P][K]
__global__ __launch_bounds__(AGG_LANES) void aggregate_lane_kernel(const uint8_t* __restrict__ labels, const AggRegion* __restrict__ regs,
                                                                   int R, int K, AggGrid gd, GroupChunks gr,
                                                                   const int32_t* __restrict__ feat, const uint8_t* __restrict__ flip,
                                                                   int tiles, int64_t nitems, unsigned long long* __restrict__ cells,
                                                                   unsigned long long* __restrict__ votes, int* __restrict__ bad) {
  extern __shared__ unsigned agg_cols[];               // [words] 16-bit histogram | [words] 16-bit votes | [2 words] u32 counts, x AGG_LANES
  const int P = gd.P, S = P * P, words = (K + 1) >> 1;
  unsigned* const hist = agg_cols + threadIdx.x;       // the lane's columns: hist[q AGG_LANES]
  unsigned* const vote = hist + words * AGG_LANES;
  unsigned* const acc = vote + words * AGG_LANES;
  for (int q = 0; q < 4 * words; ++q) hist[q * AGG_LANES] = 0;
  int wrong = 0;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t chunk = item / tiles;
    const int tile = (int)(item - chunk * tiles);
    int g = 0;
    while (g < MAX_GROUPS - 1 && gr.chunk0[g + 1] <= chunk) ++g;                    // (chunk < chunk0[G]; an empty group has no chunk)
    const int64_t a = gr.first[g] + (chunk - gr.chunk0[g]) * AGG_CHUNK;
    const int64_t b = a + AGG_CHUNK < gr.first[g + 1] ? a + AGG_CHUNK : gr.first[g + 1];
    const int cell = tile * AGG_LANES + (int)threadIdx.x;
    const bool live = cell < S;
    const int u = cell / P, v = cell - u * P;
    for (int64_t f = a; f < b; ++f) {
      AggFeature ft;
      if (!agg_feature(feat, flip, f, gd, regs, R, &ft, &wrong) || !ft.small || !live) continue;
      long long il, ih, jl, jh;
      agg_cell(ft.A, ft.flip ? P - 1 - u : u, gd, &il, &ih);
      agg_cell(ft.B, ft.flip ? P - 1 - v : v, gd, &jl, &jh);
      bool any = false;
      for (unsigned long long m = ft.mask; m; m &= m - 1) {
        const AggRegion rg = regs[__builtin_ctzll(m)];
        const uint8_t* const lab = labels + rg.lo;
#pragma unroll
        for (int mirror = 0; mirror < 2; ++mirror) {   // I x J, then J x I without the bin pairs (p, p)
          int i0, i1, j0, j1;
          if (!agg_clip(rg, mirror ? jl : il, mirror ? jh : ih, mirror ? il : jl, mirror ? ih : jh, &i0, &i1, &j0, &j1)) continue;
          for (int i = i0; i < i1; ++i) {
            const int ja = (rg.diagonal && j0 < i) ? i : j0;                         // (i < i1 <= j1 in a diagonal block)
            const uint8_t* const p = lab + grid_id<int64_t>(i, ja, rg.W, rg.diagonal);
            const int same = mirror ? rg.s1 + i - rg.s2 : -1;                        // the column of the bin pair (p, p); columns are >= 0
            for (int j = ja; j < j1; ++j) {
              if (j == same) continue;
              const int s = p[j - ja];
              if (s >= K) {
                wrong |= BAD_LABEL;
                continue;
              }
              packed_bump<AGG_LANES>(hist, s);
              any = true;
            }
          }
        }
      }
      if (!any) continue;
      unsigned best_n = 0;
      int best = 0;
      for (int q = 0; q < words; ++q) {                // ascending states and a strict >: the lowest state wins a tie
        const unsigned n = hist[q * AGG_LANES];
        if (!n) continue;
        const unsigned n0 = n & 0xffffu, n1 = n >> 16;
        if (n0 > best_n) {
          best_n = n0;
          best = 2 * q;
        }
        if (n1 > best_n) {
          best_n = n1;
          best = 2 * q + 1;
        }
        acc[(2 * q) * AGG_LANES] += n0;
        acc[(2 * q + 1) * AGG_LANES] += n1;
        hist[q * AGG_LANES] = 0;
      }
      packed_bump<AGG_LANES>(vote, best);
    }
    if (live) {
      const size_t at = ((size_t)g * S + cell) * K;
      packed_flush<AGG_LANES>(vote, words, votes + at);
      for (int k = 0; k < K; ++k) {
        const unsigned n = acc[k * AGG_LANES];
        if (n) {
          atomicAdd(cells + at + k, (unsigned long long)n);
          acc[k * AGG_LANES] = 0;
        }
      }
    }
  }
  if (wrong) atomicOr(bad, wrong);
}

__global__ __launch_bounds__(64 * AGG_WAVES) void aggregate_wave_kernel(const uint8_t* __restrict__ labels,
                                                                       const AggRegion* __restrict__ regs, int R, int K, AggGrid gd,
                                                                       GroupChunks gr, const int32_t* __restrict__ feat,
                                                                       const uint8_t* __restrict__ flip, int64_t nitems,
                                                                       unsigned long long* __restrict__ cells,
                                                                       unsigned long long* __restrict__ votes, int* __restrict__ bad) {
  __shared__ unsigned hist_all[AGG_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, P = gd.P;
  unsigned* const hist = hist_all[wave];
  hist[lane] = 0;
  wave_order();
  int wrong = 0, ignore = 0;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t f = item / P;
    const int u = (int)(item - f * P);
    AggFeature ft;
    // (the lane kernel sees every feature and reports the malformed ones)
    if (!agg_feature(feat, flip, f, gd, regs, R, &ft, &ignore) || ft.small) continue;
    const int g = group_of_entry(gr, f);
    long long il, ih;
    agg_cell(ft.A, ft.flip ? P - 1 - u : u, gd, &il, &ih);
    for (int v = wave; v < P; v += AGG_WAVES) {
      long long jl, jh;
      agg_cell(ft.B, ft.flip ? P - 1 - v : v, gd, &jl, &jh);
      unsigned long long total = 0;                    // lane k: the cell's nodes in state k
      for (unsigned long long m = ft.mask; m; m &= m - 1) {
        const AggRegion rg = regs[__builtin_ctzll(m)];
        const uint8_t* const lab = labels + rg.lo;
        for (int mirror = 0; mirror < 2; ++mirror) {   // I x J, then J x I without the bin pairs (p, p)
          int i0, i1, j0, j1;
          if (!agg_clip(rg, mirror ? jl : il, mirror ? jh : ih, mirror ? il : jl, mirror ? ih : jh, &i0, &i1, &j0, &j1)) continue;
          for (int i = i0; i < i1; ++i) {
            const int same = mirror ? rg.s1 + i - rg.s2 : -1;
            auto key_of = [&](int s, int j) -> int {
              if (j == same) return -1;
              if (s >= K) {
                wrong |= BAD_LABEL;
                return -1;
              }
              return s;
            };
            for (int jb = (rg.diagonal && j0 < i) ? i : j0; jb < j1; jb += AGG_ROW_W) {       // (i < i1 <= j1 in a diagonal block)
              const LabelRow r = label_row(lab, i, jb, jb + AGG_ROW_W < j1 ? jb + AGG_ROW_W : j1, rg.W, rg.diagonal);
              uint32_t word = 0;
              int single = 0;
              load_row(r, lane, &word, &single);
              if (r.nvec > 0) {
                int key[4] = {-1, -1, -1, -1};
                if (lane < r.nvec) {
#pragma unroll
                  for (int e = 0; e < 4; ++e) key[e] = key_of((int)((word >> (8 * e)) & 0xff), r.ja + r.head + 4 * lane + e);
                }
                wave_quad_add(hist, key);
              }
              if (r.nbytes > 0) {
                int key = -1;
                if (lane < r.nbytes) key = key_of(single, r.ja + r.byte_at(lane));
                wave_run_add(hist, key, key >= 0 ? 1u : 0u);
              }
            }
          }
          wave_order();                            // a clipped rectangle has fewer than 2^31 nodes: no bin has carried
          total += hist[lane];
          hist[lane] = 0;
          wave_order();
        }
      }
      if (lane >= K) total = 0;                        // (no key is >= K: those bins stayed 0 anyway)
      unsigned long long best_n = total;
      int best = lane;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long n = __shfl_xor(best_n, off, 64);
        const int k = __shfl_xor(best, off, 64);
        if (n > best_n || (n == best_n && k < best)) {
          best_n = n;
          best = k;
        }
      }
      if (best_n) {
        const size_t at = ((size_t)g * P * P + (size_t)u * P + v) * K;
        if (total) atomicAdd(cells + at + lane, total);
        if (lane == 0) atomicAdd(votes + at + best, 1ull);
      }
    }
  }
  if (wrong) atomicOr(bad, wrong);
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_state_aggregate(const uint8_t* labels_dev, int64_t n_labels, int R, const int64_t* regions_host, int K, int T, int F, int G,
                          const int64_t* group_offsets_host, const int32_t* feat_dev, const uint8_t* flip_dev_or_null,
                          int64_t* cells_host, int64_t* votes_host, void* hip_stream) {
  PHMRF_CHECK(labels_dev && regions_host && group_offsets_host && cells_host && votes_host, PHMRF_ERR_INVALID,
              "NULL labels, regions, group offsets or output table");
  PHMRF_CHECK(n_labels >= 1, PHMRF_ERR_INVALID, "n_labels must be >= 1");
  PHMRF_CHECK(R >= 1, PHMRF_ERR_INVALID, "R must be >= 1");
  PHMRF_CHECK(K >= 1, PHMRF_ERR_INVALID, "K must be >= 1");
  PHMRF_CHECK(T >= 1, PHMRF_ERR_INVALID, "T must be >= 1");
  PHMRF_CHECK(F >= 0, PHMRF_ERR_INVALID, "F must be >= 0");
  PHMRF_CHECK(G >= 1, PHMRF_ERR_INVALID, "G must be >= 1");
  PHMRF_TRY(check_states(K));
  PHMRF_CHECK(T <= AGG_MAX_BODY, PHMRF_ERR_UNSUPPORTED, "T must be <= 64");
  PHMRF_CHECK(F <= AGG_MAX_FLANK, PHMRF_ERR_UNSUPPORTED, "F must be <= 32");
  PHMRF_CHECK(G <= MAX_GROUPS, PHMRF_ERR_UNSUPPORTED, "G must be <= 16");
  PHMRF_CHECK(R <= AGG_MAX_REGIONS, PHMRF_ERR_UNSUPPORTED, "R must be <= 64");
  const int P = T + 2 * F, S = P * P;
  const int64_t n_tab = (int64_t)G * S * K;
  PHMRF_CHECK(n_tab <= AGG_MAX_TABLE, PHMRF_ERR_UNSUPPORTED, "G (T + 2 F)^2 K must be <= 2^24");
  std::vector<AggRegion> regs((size_t)R);
  for (int r = 0; r < R; ++r) {
    const int64_t* row = regions_host + 6 * (size_t)r;
    PHMRF_CHECK(row[1] >= 1 && row[2] >= 1, PHMRF_ERR_INVALID, "H and W must be >= 1");
    PHMRF_CHECK(row[1] < ((int64_t)1 << 31) && row[2] < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED, "H and W must be below 2^31");
    PHMRF_CHECK(row[5] == 0 || row[5] == 1, PHMRF_ERR_INVALID, "diagonal must be 0 or 1");
    int64_t n = 0;
    PHMRF_TRY(check_region((int)row[1], (int)row[2], (int)row[5], &n));
    PHMRF_TRY(check_nodes(n));
    PHMRF_CHECK(row[0] >= 0 && row[0] + n <= n_labels, PHMRF_ERR_INVALID, "a region's nodes must lie inside the labels");
    PHMRF_CHECK(row[3] >= 0 && row[4] >= 0, PHMRF_ERR_INVALID, "a region's start bins must be >= 0");
    PHMRF_CHECK(!coord_out(row[3]) && !coord_out(row[4]), PHMRF_ERR_UNSUPPORTED, "a region's start bins must be below 2^30");
    regs[(size_t)r] = AggRegion{(long long)row[0], (int)row[1], (int)row[2], (int)row[3], (int)row[4], (int)row[5], 0};
  }
  GroupChunks gr;
  int64_t N = 0;
  PHMRF_TRY(group_first(group_offsets_host, G, "features", &gr, &N));
  PHMRF_CHECK(N == 0 || feat_dev, PHMRF_ERR_INVALID, "NULL features");
  if (N == 0) {
    for (int64_t t = 0; t < n_tab; ++t) cells_host[t] = votes_host[t] = 0;
    return PHMRF_OK;
  }
  group_chunks(&gr, AGG_CHUNK);
  const int tiles = (S + AGG_LANES - 1) / AGG_LANES;
  const int64_t lane_items = gr.chunk0[G] * tiles, wave_items = N * P;
  const AggGrid gd{T, F, P, (int)((((int64_t)1 << 24) + T - 1) / T)};

  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  Buffers buf;
  FlaggedTable tab(st);                                // cells | votes
  AggRegion* regs_dev;
  PHMRF_TRY(tab.make(&buf, (size_t)(2 * n_tab)));
  PHMRF_TRY(buf.get(&regs_dev, (size_t)R));
  unsigned long long* const table = tab.words();
  PHMRF_HIP(hipMemcpyAsync(regs_dev, regs.data(), (size_t)R * sizeof(AggRegion), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(aggregate_lane_kernel, dim3(grid_of(lane_items, 1, AGG_GRID_CAP)), dim3(AGG_LANES), aggregate_lds_bytes(K), st,
                     labels_dev, regs_dev, R, K, gd, gr, feat_dev, flip_dev_or_null, tiles, lane_items, table, table + n_tab, tab.flag());
  PHMRF_HIP(hipGetLastError());
  hipLaunchKernelGGL(aggregate_wave_kernel, dim3(grid_of(wave_items, 1, AGG_WAVE_GRID_CAP)), dim3(64 * AGG_WAVES), 0, st, labels_dev,
                     regs_dev, R, K, gd, gr, feat_dev, flip_dev_or_null, wave_items, table, table + n_tab, tab.flag());
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_TRY(tab.read_flag(&bad));
  PHMRF_CHECK(!(bad & BAD_FLIP), PHMRF_ERR_INVALID, "a flip is > 1");
  PHMRF_CHECK(!(bad & BAD_COORD), PHMRF_ERR_UNSUPPORTED, "a feature coordinate has |c| >= 2^30");
  PHMRF_CHECK(!(bad & BAD_EMPTY), PHMRF_ERR_INVALID, "a feature needs a1 > a0 and b1 > b0");
  PHMRF_CHECK(!(bad & BAD_LABEL), PHMRF_ERR_INVALID, "a label inside a feature's cell is >= K");
  PHMRF_TRY(tab.copy(0, (size_t)n_tab, cells_host));
  PHMRF_TRY(tab.copy((size_t)n_tab, (size_t)n_tab, votes_host));
  return tab.wait();
}

}  // extern "C"
