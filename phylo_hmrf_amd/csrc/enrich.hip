// gfx950 kernels that count the states of ONE region's bin pairs against the annotation of their two bins and against
// their exact genomic distance (phmrf_pair_enrichment).  Integer arithmetic throughout: no result
// depends on the order in which the atomics land.
//
//   labels   obs[p][k] and state_dist[d - d_lo][k] over the stored nodes INSIDE the distance window.  A workgroup owns a TILE
//            of ENRICH_TILE_H storage rows by ENRICH_TILE_W storage columns, the tiles stride over a capped grid; a tile
//            wholly outside the window is left without a load, a tile wholly inside it drops the per-cell test (as
//            tracks.hip).  A HALF-wave holds one storage row: up to three head bytes to the next 4-byte boundary of the
//            row's address, one 4-byte load per lane (four labels), up to three tail bytes (label_row, runs.h; the tile's
//            geometry and the row a half-wave counts: enrich_tiles.h, with enrich_null.hip).  The tile's class and segment of every
//            row and column bin are staged in LDS once (8 bytes a bin).
//            obs: u32 [P][K] in LDS for the workgroup's whole life, ONE atomic per run of equal (p, k) among consecutive
//            lanes (wave_run_add; a run may cross the two rows of a wave, the sum is the same), flushed at the end with u64
//            global atomics on the non-zero bins.
//            state_dist: the tile's distances are [near, near + ENRICH_TILE_D): dist0 + j - i takes at most TILE_H + TILE_W
//            - 1 values over a tile, and where the tile straddles 0 the values x and -x fold onto one distance.  A signed
//            diagonal has at most TILE_H cells in a tile, a (distance, state) bin of one tile so at most 2 TILE_H = 64: 16-bit
//            counters, two states to a word, a row stride of an odd number of words.  One atomic per cell; the lanes take
//            their four columns in a rotated order (lane >> 3), so that 32 lanes of one state fall on 32 banks instead of 8.
//            Flushed per tile with u32 global atomics on the non-zero counters.
//   classes  cat_dist[d - d_lo][p]: no labels are read.  A wave takes ENRICH_CHUNK consecutive rows i of ONE signed diagonal
//            x = dist0 + j - i inside the window, lane <-> i, 64 at a time; p changes at interval borders only, so
//            wave_run_add into the wave's own [P] table in LDS takes a handful of atomics; the table goes to
//            cat_dist[|x| - d_lo] with u32 global atomics when the chunk is done.  A diagonal block visits x >= 0.
//   A label >= K inside the window sets bit 0 of the flag word, a class >= C on a node inside the window bit 1; nodes outside
//   the window are not inspected.

#include "enrich_tiles.h"

namespace phmrf {
namespace {

constexpr int ENRICH_GRID_CAP = 1024;    // workgroups of either kernel (enrich.py GRID_CAP)
constexpr int ENRICH_CHUNK = 512;        // cells of a diagonal a wave of the class kernel takes at a time

// u32 words of a distance's row of the tile table: two states to a word, odd
__host__ __device__ __forceinline__ int enrich_dist_stride(int K) { return ((K + 1) / 2) | 1; }

// LDS of the label kernel: class and segment of the tile's bins (8 bytes each), obs, the tile's distance table
inline size_t enrich_lds_bytes(int K, int C) {
  return 8 * (size_t)(ENRICH_TILE_W + ENRICH_TILE_H) + 4 * ((size_t)2 * C * C * K + (size_t)ENRICH_TILE_D * enrich_dist_stride(K));
}

// obs: u64 [2 C C][K]; state_dist: u32 [D][K], row 0 the distance tab_lo; d_hi: INT_MAX for no upper limit.  col_class /
// col_seg: the row arrays again for a diagonal block; row_seg and col_seg both null without segments.
__global__ __launch_bounds__(256) void enrich_label_kernel(const uint8_t* __restrict__ labels, int H, int W, int diagonal, int dist0,
                                                           int K, int C, const uint8_t* __restrict__ row_class,
                                                           const uint8_t* __restrict__ col_class,
                                                           const int32_t* __restrict__ row_seg, const int32_t* __restrict__ col_seg,
                                                           int d_lo, int d_hi, int tab_lo, int per_row, int64_t ntiles,
                                                           unsigned long long* __restrict__ obs, unsigned* __restrict__ state_dist,
                                                           int* __restrict__ bad) {
  extern __shared__ int2 enrich_lds[];
  int2* const col_info = enrich_lds;                                   // (class, segment) of the tile's columns ...
  int2* const row_info = enrich_lds + ENRICH_TILE_W;                   // ... and rows
  unsigned* const obs_tab = reinterpret_cast<unsigned*>(enrich_lds + ENRICH_TILE_W + ENRICH_TILE_H);
  const int ds = enrich_dist_stride(K), nobs = 2 * C * C * K;
  unsigned* const dist_tab = obs_tab + nobs;
  for (int t = threadIdx.x; t < nobs + ENRICH_TILE_D * ds; t += 256) obs_tab[t] = 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l32 = lane & 31;
  const int rot = (l32 >> 3) & 3;
  int wrong = 0;
  for (int64_t T = blockIdx.x; T < ntiles; T += gridDim.x) {
    WindowTile t;                                      // (its distances: nd <= ENRICH_TILE_D)
    if (!window_tile<ENRICH_TILE_H, ENRICH_TILE_W>(T, H, W, diagonal, per_row, dist0, d_lo, d_hi, &t)) continue;
    uint32_t word[ENRICH_PAIRS_PER_WAVE];
    int single[ENRICH_PAIRS_PER_WAVE];
    load_tile_rows<8>(labels, t, W, diagonal, 2 * wave + half, l32, word, single);   // a half-wave per row
    if (threadIdx.x < ENRICH_TILE_W) {
      const int j = t.j0 + threadIdx.x;
      if (j < t.j1) col_info[threadIdx.x] = make_int2(col_class[j], col_seg ? col_seg[j] : -1);
    } else if (threadIdx.x < ENRICH_TILE_W + ENRICH_TILE_H) {
      const int i = t.i0 + (threadIdx.x - ENRICH_TILE_W);
      if (i < t.i1) row_info[i - t.i0] = make_int2(row_class[i], row_seg ? row_seg[i] : -1);
    }
    __syncthreads();                                   // (the first tile: the zeroed tables too)
#pragma unroll
    for (int u = 0; u < ENRICH_PAIRS_PER_WAVE; ++u) {
      if (t.i0 + 2 * wave + 8 * u >= t.i1) break;       // the same for the wave; its second row may still be absent
      const int i = t.i0 + 2 * wave + half + 8 * u;
      const bool present = i < t.i1;
      const LabelRow r = present_row(labels, t, i, present, W, diagonal);
      const int2 mine = row_info[present ? i - t.i0 : 0];
      const int x0 = dist0 - i;                         // the cell's distance is |x0 + j|
      // one cell: -1 outside the window, with a label >= K or a class >= C, else its obs bin; the distance table takes it here
      auto cell = [&](int s, int j) -> int {
        const int x = x0 + j, d = x < 0 ? -x : x;
        if (!t.whole && (d < d_lo || d > d_hi)) return -1;
        if (s >= K) {
          wrong |= BAD_LABEL;
          return -1;
        }
        const int2 other = col_info[j - t.j0];
        if (mine.x >= C || other.x >= C) {
          wrong |= BAD_CLASS;
          return -1;
        }
        atomicAdd(dist_tab + (d - t.near) * ds + (s >> 1), 1u << (16 * (s & 1)));
        return pair_bin(mine, other, C) * K + s;
      };
      {
        int key[4] = {-1, -1, -1, -1};
        if (l32 < r.nvec) {
          const uint32_t w = __builtin_rotateright32(word[u], 8 * rot);
          const int j = r.ja + r.head + 4 * l32;
#pragma unroll
          for (int e = 0; e < 4; ++e) key[e] = cell((int)((w >> (8 * e)) & 0xff), j + ((e + rot) & 3));
        }
        wave_quad_add(obs_tab, key);
      }
      {
        int key = -1;
        if (l32 < r.nbytes) key = cell(single[u], r.ja + r.byte_at(l32));
        wave_run_add(obs_tab, key, key >= 0 ? 1u : 0u);
      }
    }
    __syncthreads();
    for (int x = threadIdx.x; x < t.nd * ds; x += 256) {
      const unsigned c = dist_tab[x];
      if (c) {
        const int dd = x / ds, s = 2 * (x - dd * ds);
        unsigned* const out = state_dist + (size_t)(t.near + dd - tab_lo) * K + s;
        if (c & 0xffffu) atomicAdd(out, c & 0xffffu);
        if (c >> 16) atomicAdd(out + 1, c >> 16);
        dist_tab[x] = 0;
      }
    }
    __syncthreads();
  }
  __syncthreads();                                     // (a workgroup without a tile: the zeroed table)
  for (int x = threadIdx.x; x < nobs; x += 256) {
    const unsigned c = obs_tab[x];
    if (c) atomicAdd(obs + x, (unsigned long long)c);
  }
  if (wrong) atomicOr(bad, wrong);
}

// cat_dist: u32 [D][2 C C], row 0 the distance tab_lo.  The diagonals and their chunks of ENRICH_CHUNK rows: diagonal_chunk.
__global__ __launch_bounds__(256) void enrich_class_kernel(int H, int W, int diagonal, int dist0, int C,
                                                           const uint8_t* __restrict__ row_class,
                                                           const uint8_t* __restrict__ col_class,
                                                           const int32_t* __restrict__ row_seg, const int32_t* __restrict__ col_seg,
                                                           int xa, int na, int xb, int slots, int64_t nitems, int tab_lo,
                                                           unsigned* __restrict__ cat_dist, int* __restrict__ bad) {
  __shared__ unsigned tabs[4][ENRICH_MAX_PAIRS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* const tab = tabs[wave];
  const int P = 2 * C * C;
  for (int q = lane; q < ENRICH_MAX_PAIRS; q += 64) tab[q] = 0;
  __syncthreads();
  bool wrong = false;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < nitems; item += (int64_t)gridDim.x * 4) {
    int x, shift, a, b;
    if (!diagonal_chunk<ENRICH_CHUNK>(item, slots, xa, na, xb, dist0, H, W, &x, &shift, &a, &b)) continue;
    for (int base = a; base < b; base += 64) {
      const int i = base + lane;
      int key = -1;
      if (i < b) {
        const int j = i + shift;
        const int rc = row_class[i], cc = col_class[j];
        if (rc >= C || cc >= C) {
          wrong = true;
        } else {
          const int rs = row_seg ? row_seg[i] : -1, cs = col_seg ? col_seg[j] : -1;
          key = pair_bin(make_int2(rc, rs), make_int2(cc, cs), C);
        }
      }
      wave_run_add(tab, key, key >= 0 ? 1u : 0u);
    }
    const int d = x < 0 ? -x : x;
    for (int q = lane; q < P; q += 64) {                // (LDS operations of one wave complete in order)
      const unsigned c = tab[q];
      if (c) {
        atomicAdd(cat_dist + (size_t)(d - tab_lo) * P + q, c);
        tab[q] = 0;
      }
    }
  }
  if (wrong) atomicOr(bad, BAD_CLASS);
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_pair_enrichment(const uint8_t* labels_dev, int H, int W, int diagonal, int64_t dist0, int K, int C,
                          const uint8_t* row_class_dev, const uint8_t* col_class_dev_or_null, const int32_t* row_seg_dev_or_null,
                          const int32_t* col_seg_dev_or_null, int64_t d_min, int64_t d_max, int64_t d_lo, int64_t D,
                          int64_t* obs_host, int64_t* state_dist_host, int64_t* cat_dist_host, void* hip_stream) {
  PHMRF_CHECK(labels_dev && row_class_dev && obs_host && state_dist_host && cat_dist_host, PHMRF_ERR_INVALID,
              "NULL labels, row classes or output table");
  int64_t n;
  PHMRF_TRY(check_region(H, W, diagonal, &n));
  PHMRF_CHECK(diagonal || col_class_dev_or_null, PHMRF_ERR_INVALID, "an off-diagonal block needs column classes");
  PHMRF_CHECK(diagonal || (row_seg_dev_or_null == nullptr) == (col_seg_dev_or_null == nullptr), PHMRF_ERR_INVALID,
              "an off-diagonal block needs row and column segments, or neither");
  PHMRF_CHECK(K >= 1 && C >= 1, PHMRF_ERR_INVALID, "K and C must be >= 1");
  PHMRF_CHECK(D >= 0 && d_lo >= 0, PHMRF_ERR_INVALID, "D and d_lo must be >= 0");
  PHMRF_CHECK(!diagonal || dist0 == 0, PHMRF_ERR_INVALID, "a diagonal block has dist0 == 0");
  PHMRF_TRY(check_window(d_min, d_max));
  PHMRF_TRY(check_states(K));                          // (its upper limit)
  PHMRF_CHECK(C <= ENRICH_MAX_CLASSES, PHMRF_ERR_UNSUPPORTED, "C must be <= 8");
  PHMRF_TRY(check_nodes(n, "n must be below 2^31 - 64"));
  PHMRF_TRY(check_span(dist0, H, W));
  const int P = 2 * C * C;
  PHMRF_CHECK(D < ((int64_t)1 << 31) && D * (K > P ? K : P) < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED,
              "D max(K, 2 C C) must be below 2^31");
  const IntWindow win = int_window(d_min, d_max);
  WindowDiagonals dg;
  PHMRF_TRY(window_diagonals(H, W, diagonal, dist0, win, d_lo, D, &dg));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const size_t n_obs = (size_t)P * K, n_sd = (size_t)D * K, n_cd = (size_t)D * P;
  if (dg.na + dg.nb == 0) {                            // nothing inside the window
    for (size_t t = 0; t < n_obs; ++t) obs_host[t] = 0;
    for (size_t t = 0; t < n_sd; ++t) state_dist_host[t] = 0;
    for (size_t t = 0; t < n_cd; ++t) cat_dist_host[t] = 0;
    return PHMRF_OK;
  }
  const uint8_t* const col_class = diagonal ? row_class_dev : col_class_dev_or_null;
  const int32_t* const col_seg = diagonal ? row_seg_dev_or_null : col_seg_dev_or_null;
  int per_row;
  const int64_t ntiles = window_tile_count<ENRICH_TILE_H, ENRICH_TILE_W>(H, W, diagonal, &per_row);
  const int slots = ((H < W ? H : W) + ENRICH_CHUNK - 1) / ENRICH_CHUNK;
  const int64_t nitems = ((int64_t)dg.na + dg.nb) * slots;

  // one allocation and one memset, whatever the call's size: obs u64 [P K] | state_dist u32 [D K] | cat_dist u32 [D P] | the flag word
  Buffers buf;
  unsigned long long* all;
  const size_t n_u32 = n_sd + n_cd + 1;
  PHMRF_TRY(buf.get(&all, n_obs + (n_u32 + 1) / 2));
  unsigned* const state_dist = reinterpret_cast<unsigned*>(all + n_obs);
  unsigned* const cat_dist = state_dist + n_sd;
  int* const flag = reinterpret_cast<int*>(cat_dist + n_cd);
  PHMRF_HIP(hipMemsetAsync(all, 0, (n_obs + (n_u32 + 1) / 2) * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(enrich_label_kernel, dim3(grid_of(ntiles, 1, ENRICH_GRID_CAP)), dim3(256), enrich_lds_bytes(K, C), st, labels_dev,
                     H, W, diagonal, (int)dist0, K, C, row_class_dev, col_class, row_seg_dev_or_null, col_seg, win.lo, win.hi,
                     (int)d_lo, per_row, ntiles, all, state_dist, flag);
  PHMRF_HIP(hipGetLastError());
  hipLaunchKernelGGL(enrich_class_kernel, dim3(grid_of(nitems, 4, ENRICH_GRID_CAP)), dim3(256), 0, st, H, W, diagonal, (int)dist0, C,
                     row_class_dev, col_class, row_seg_dev_or_null, col_seg, dg.xa, dg.na, dg.xb, slots, nitems, (int)d_lo,
                     cat_dist, flag);
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  PHMRF_CHECK(!(bad & BAD_LABEL), PHMRF_ERR_INVALID, "a label inside the window is >= K");
  PHMRF_CHECK(!(bad & BAD_CLASS), PHMRF_ERR_INVALID, "a class of a node inside the window is >= C");
  std::vector<unsigned long long> got(n_obs + (n_sd + n_cd + 1) / 2);          // the three tables in one copy
  PHMRF_HIP(hipMemcpyAsync(got.data(), all, n_obs * sizeof(unsigned long long) + (n_sd + n_cd) * sizeof(unsigned),
                           hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  const unsigned* const got_u32 = reinterpret_cast<const unsigned*>(got.data() + n_obs);
  for (size_t t = 0; t < n_obs; ++t) obs_host[t] = (int64_t)got[t];
  for (size_t t = 0; t < n_sd; ++t) state_dist_host[t] = (int64_t)got_u32[t];
  for (size_t t = 0; t < n_cd; ++t) cat_dist_host[t] = (int64_t)got_u32[n_sd + t];
  return PHMRF_OK;
}

}  // extern "C"
