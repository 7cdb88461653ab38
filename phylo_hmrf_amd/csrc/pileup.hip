// gfx950 kernel that piles ONE region's state map up around a list of centres (phmrf_state_pileup):
// obs[g][u + w][v + w][k] = the centres of group g whose pile cell (u, v) lies on a cell of the region's full matrix in state
// k.  Integer arithmetic throughout: no result depends on the order in which the atomics land.
//
//   An ITEM is a tile of PILEUP_LANES consecutive pile cells (v fastest) times a CHUNK of at most PILEUP_CHUNK consecutive
//   centres of ONE group; the items (the tile fastest, so that neighbouring workgroups walk the same centres) stride over a
//   capped grid.  The groups' offsets and first chunks travel in the kernel's arguments (GroupChunks, interval_lists.h).
//   lane <-> pile cell: for an untransposed centre the 64 lanes of a wave read contiguous pieces of at most two storage rows.
//   The centre is the same for every lane (uniform loads), the label a one-byte gather; four centres' labels are loaded before
//   the first of them is counted.  A centre whose whole window misses the region is passed over without a load.
//   Every lane keeps a private column of 16-bit counters in LDS (packed_bump / packed_flush, interval_lists.h; a chunk has at
//   most 256 centres: a counter never carries): no LDS atomics, no bank conflicts and no barrier anywhere in the kernel.  At
//   K = 64 the columns take 32 KB.  After the chunk a lane adds its non-zero counters to the device table and zeroes them.
//   The label check is as in tracks.hip and enrich.hip: only a cell some window holds is looked at.  Flag bits: a label >= K
//   on such a cell, an orient > 3, a coordinate with |c| >= 2^30 (such a centre is passed over).
//   label_row (runs.h) does not fit: it describes a contiguous piece of ONE storage row per half-wave, the pile reads a
//   single byte per lane and centre.

#include "interval_lists.h"

namespace phmrf {
namespace {

constexpr int PILEUP_LANES = 256;        // pile cells of a tile = lanes of a workgroup (pileup.py LANES)
constexpr int PILEUP_CHUNK = 256;        // centres of one group a workgroup piles before it adds to the table (pileup.py CHUNK)
constexpr int PILEUP_GRID_CAP = 4096;    // workgroups (pileup.py GRID_CAP)
constexpr int PILEUP_MAX_FLANK = 64;     // w <= 64 (pileup.py MAX_FLANK)
constexpr int PILEUP_BATCH = 4;          // centres whose labels are in flight together
constexpr int BAD_LABEL = 1, BAD_ORIENT = 2, BAD_COORD = 4;

static_assert(PILEUP_CHUNK < 65536, "a 16-bit counter holds a chunk");

inline size_t pileup_lds_bytes(int K) { return (size_t)((K + 1) / 2) * PILEUP_LANES * sizeof(unsigned); }

// table: u64 [G][side side][K]
__global__ __launch_bounds__(PILEUP_LANES) void pileup_kernel(const uint8_t* __restrict__ labels, int H, int W, int diagonal, int K,
                                                              int w, GroupChunks gr, const int32_t* __restrict__ ci,
                                                              const int32_t* __restrict__ cj, const uint8_t* __restrict__ orient,
                                                              int tiles, int64_t nitems, unsigned long long* __restrict__ table,
                                                              int* __restrict__ bad) {
  extern __shared__ unsigned pile_cols[];              // [(K + 1) / 2][PILEUP_LANES]
  const int side = 2 * w + 1, S = side * side, words = (K + 1) >> 1;
  unsigned* const mine = pile_cols + threadIdx.x;      // the lane's column: mine[q PILEUP_LANES]
  for (int q = 0; q < words; ++q) mine[q * PILEUP_LANES] = 0;
  int wrong = 0;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t chunk = item / tiles;
    const int tile = (int)(item - chunk * tiles);
    int g = 0;
    while (g < MAX_GROUPS - 1 && gr.chunk0[g + 1] <= chunk) ++g;                    // (chunk < chunk0[G]; an empty group has no chunk)
    const int64_t a = gr.first[g] + (chunk - gr.chunk0[g]) * PILEUP_CHUNK;
    const int64_t b = a + PILEUP_CHUNK < gr.first[g + 1] ? a + PILEUP_CHUNK : gr.first[g + 1];
    const int cell = tile * PILEUP_LANES + (int)threadIdx.x;
    const bool live = cell < S;
    const int u = cell / side - w, v = cell - (cell / side) * side - w;
    for (int64_t c = a; c < b; c += PILEUP_BATCH) {
      int s[PILEUP_BATCH];
#pragma unroll
      for (int e = 0; e < PILEUP_BATCH; ++e) {
        s[e] = -1;
        if (c + e >= b) continue;
        const int ai = ci[c + e], aj = cj[c + e];
        const int o = orient ? orient[c + e] : 0;
        if (o > 3) wrong |= BAD_ORIENT;
        if (coord_out(ai) || coord_out(aj)) {
          wrong |= BAD_COORD;
          continue;
        }
        if (ai + w < 0 || ai - w >= H || aj + w < 0 || aj - w >= W) continue;          // the window misses the region
        const int p = (o & 2) ? v : u, q = (o & 2) ? u : v;
        int i = (o & 1) ? ai - p : ai + p, j = (o & 1) ? aj - q : aj + q;
        if (!live || i < 0 || i >= H || j < 0 || j >= W) continue;
        if (diagonal && i > j) {
          const int t = i;
          i = j;
          j = t;
        }
        s[e] = labels[grid_id<int64_t>(i, j, W, diagonal)];
      }
#pragma unroll
      for (int e = 0; e < PILEUP_BATCH; ++e) {
        if (s[e] < 0) continue;
        if (s[e] >= K) {
          wrong |= BAD_LABEL;
          continue;
        }
        packed_bump<PILEUP_LANES>(mine, s[e]);
      }
    }
    if (live) packed_flush<PILEUP_LANES>(mine, words, table + ((size_t)g * S + cell) * K);
  }
  if (wrong) atomicOr(bad, wrong);
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_state_pileup(const uint8_t* labels_dev, int H, int W, int diagonal, int K, int w, int G,
                       const int64_t* group_offsets_host, const int32_t* ci_dev, const int32_t* cj_dev,
                       const uint8_t* orient_dev_or_null, int64_t* obs_host, void* hip_stream) {
  PHMRF_CHECK(labels_dev && group_offsets_host && obs_host, PHMRF_ERR_INVALID, "NULL labels, group offsets or output table");
  int64_t n = 0;
  PHMRF_TRY(check_region(H, W, diagonal, &n));
  PHMRF_CHECK(K >= 1, PHMRF_ERR_INVALID, "K must be >= 1");
  PHMRF_CHECK(w >= 0, PHMRF_ERR_INVALID, "w must be >= 0");
  PHMRF_CHECK(G >= 1, PHMRF_ERR_INVALID, "G must be >= 1");
  PHMRF_TRY(check_states(K));
  PHMRF_CHECK(w <= PILEUP_MAX_FLANK, PHMRF_ERR_UNSUPPORTED, "w must be <= 64");
  PHMRF_CHECK(G <= MAX_GROUPS, PHMRF_ERR_UNSUPPORTED, "G must be <= 16");
  PHMRF_TRY(check_nodes(n, "n must be below 2^31 - 64"));
  GroupChunks gr;
  int64_t n_centres = 0;
  PHMRF_TRY(group_first(group_offsets_host, G, "centres", &gr, &n_centres));
  PHMRF_CHECK(n_centres == 0 || (ci_dev && cj_dev), PHMRF_ERR_INVALID, "NULL centre coordinates");
  const int side = 2 * w + 1, S = side * side;
  const size_t n_obs = (size_t)G * S * K;
  if (n_centres == 0) {
    for (size_t t = 0; t < n_obs; ++t) obs_host[t] = 0;
    return PHMRF_OK;
  }
  group_chunks(&gr, PILEUP_CHUNK);
  const int tiles = (S + PILEUP_LANES - 1) / PILEUP_LANES;
  const int64_t nitems = gr.chunk0[G] * tiles;

  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  Buffers buf;
  FlaggedTable tab(st);
  PHMRF_TRY(tab.make(&buf, n_obs));
  hipLaunchKernelGGL(pileup_kernel, dim3(grid_of(nitems, 1, PILEUP_GRID_CAP)), dim3(PILEUP_LANES), pileup_lds_bytes(K), st, labels_dev,
                     H, W, diagonal, K, w, gr, ci_dev, cj_dev, orient_dev_or_null, tiles, nitems, tab.words(), tab.flag());
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_TRY(tab.read_flag(&bad));
  PHMRF_CHECK(!(bad & BAD_ORIENT), PHMRF_ERR_INVALID, "an orient is > 3");
  PHMRF_CHECK(!(bad & BAD_COORD), PHMRF_ERR_UNSUPPORTED, "a centre coordinate has |c| >= 2^30");
  PHMRF_CHECK(!(bad & BAD_LABEL), PHMRF_ERR_INVALID, "a label inside a centre's window is >= K");
  PHMRF_TRY(tab.copy(0, n_obs, obs_host));
  return tab.wait();
}

}  // extern "C"
