// gfx950 kernels that count the states of ONE region's bin pairs against the annotation of their two bins and against
// their exact genomic distance (phmrf_pair_enrichment).  Integer arithmetic throughout: no result
// depends on the order in which the atomics land.
//
//   labels   obs[p][k] and state_dist[d - d_lo][k] over the stored nodes INSIDE the distance window.  A workgroup owns a TILE
//            of ENRICH_TILE_H storage rows by ENRICH_TILE_W storage columns, the tiles stride over a capped grid; a tile
//            wholly outside the window is left without a load, a tile wholly inside it drops the per-cell test (as
//            tracks.hip).  A HALF-wave holds one storage row: up to three head bytes to the next 4-byte boundary of the
//            row's address, one 4-byte load per lane (four labels), up to three tail bytes (label_row, runs.h).  The tile's class and segment
//            of every row and column bin are staged in LDS once (8 bytes a bin).
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

#include "runs.h"

#include <climits>

namespace phmrf {
namespace {

constexpr int ENRICH_GRID_CAP = 1024;    // workgroups of either kernel (enrich.py GRID_CAP)
constexpr int ENRICH_TILE_H = 32;        // storage rows of a tile (enrich.py TILE_H)
constexpr int ENRICH_TILE_W = 128;       // storage columns of a tile: 32 lanes x 4 labels (enrich.py TILE_W)
constexpr int ENRICH_TILE_D = ENRICH_TILE_H + ENRICH_TILE_W - 1;   // distances of a tile
constexpr int ENRICH_PAIRS_PER_WAVE = ENRICH_TILE_H / 8;           // a workgroup is four waves of two rows each
constexpr int ENRICH_PER_SUPER = ENRICH_TILE_W / ENRICH_TILE_H;    // tiles of a square super-tile (diagonal blocks)
constexpr int ENRICH_CHUNK = 512;        // cells of a diagonal a wave of the class kernel takes at a time
constexpr int ENRICH_MAX_CLASSES = 8;
constexpr int ENRICH_MAX_PAIRS = 2 * ENRICH_MAX_CLASSES * ENRICH_MAX_CLASSES;
constexpr int BAD_LABEL = 1, BAD_CLASS = 2;

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
    // the half-wave's rows i0 + 2 wave + half, + 8, ...: every load of the tile is issued before the first count
    uint32_t word[ENRICH_PAIRS_PER_WAVE];
    int single[ENRICH_PAIRS_PER_WAVE];
#pragma unroll
    for (int u = 0; u < ENRICH_PAIRS_PER_WAVE; ++u) {
      const int i = t.i0 + 2 * wave + half + 8 * u;
      word[u] = 0;
      single[u] = 0;
      if (i < t.i1) {
        const LabelRow r = label_row(labels, i, t.j0, t.j1, W, diagonal);
        if (l32 < r.nvec) word[u] = *reinterpret_cast<const uint32_t*>(r.p + r.head + 4 * l32);
        if (l32 < r.nbytes) single[u] = r.p[l32 < r.head ? l32 : r.tail + (l32 - r.head)];
      }
    }
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
      LabelRow r = label_row(labels, present ? i : t.i0, t.j0, t.j1, W, diagonal);
      if (!present) r.nvec = r.nbytes = 0;
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
        const int same = (mine.y >= 0 && mine.y == other.y) ? 1 : 0;
        atomicAdd(dist_tab + (d - t.near) * ds + (s >> 1), 1u << (16 * (s & 1)));
        return ((mine.x * C + other.x) * 2 + same) * K + s;
      };
      {
        int key[4] = {-1, -1, -1, -1};
        if (l32 < r.nvec) {
          const uint32_t w = __builtin_rotateright32(word[u], 8 * rot);
          const int j = r.ja + r.head + 4 * l32;
#pragma unroll
          for (int e = 0; e < 4; ++e) key[e] = cell((int)((w >> (8 * e)) & 0xff), j + ((e + rot) & 3));
        }
        unsigned lead = key[0] >= 0 ? 1u : 0u;          // the lane's cells in the bin of its first
        int e = 1;
        for (; e < 4 && lead && key[e] == key[0]; ++e) ++lead;
        wave_run_add(obs_tab, key[0], lead);
        for (; e < 4; ++e)
          if (key[e] >= 0) atomicAdd(obs_tab + key[e], 1u);
      }
      {
        int key = -1;
        if (l32 < r.nbytes) key = cell(single[u], r.ja + (l32 < r.head ? l32 : r.tail + (l32 - r.head)));
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

// cat_dist: u32 [D][2 C C], row 0 the distance tab_lo.  The diagonals: x = xa + t for t < na, x = xb + (t - na) for the nb
// after them; `slots` chunks of ENRICH_CHUNK rows cover the longest diagonal; item = t slots + slot.
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
    const int t = (int)(item / slots), slot = (int)(item - (int64_t)t * slots);
    const int x = t < na ? xa + t : xb + (t - na);
    // the rows i of the diagonal: 0 <= i < H and 0 <= j = i + x - dist0 < W
    const int shift = x - dist0;                        // in [-(H - 1), W - 1]
    const int i_lo = shift < 0 ? -shift : 0, i_hi = W - shift < H ? W - shift : H;
    const int64_t a64 = (int64_t)i_lo + (int64_t)slot * ENRICH_CHUNK;
    if (a64 >= i_hi) continue;                          // (the same for the wave)
    const int a = (int)a64, b = i_hi - a > ENRICH_CHUNK ? a + ENRICH_CHUNK : i_hi;
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
          key = (rc * C + cc) * 2 + ((rs >= 0 && rs == cs) ? 1 : 0);
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
  PHMRF_CHECK(diagonal == 0 || diagonal == 1, PHMRF_ERR_INVALID, "diagonal must be 0 or 1");
  PHMRF_CHECK(diagonal || col_class_dev_or_null, PHMRF_ERR_INVALID, "an off-diagonal block needs column classes");
  PHMRF_CHECK(diagonal || (row_seg_dev_or_null == nullptr) == (col_seg_dev_or_null == nullptr), PHMRF_ERR_INVALID,
              "an off-diagonal block needs row and column segments, or neither");
  PHMRF_CHECK(H >= 1 && W >= 1, PHMRF_ERR_INVALID, "H and W must be >= 1");
  PHMRF_CHECK(K >= 1 && C >= 1, PHMRF_ERR_INVALID, "K and C must be >= 1");
  PHMRF_CHECK(D >= 0 && d_lo >= 0, PHMRF_ERR_INVALID, "D and d_lo must be >= 0");
  PHMRF_CHECK(!diagonal || H == W, PHMRF_ERR_INVALID, "a diagonal block is square (H == W)");
  PHMRF_CHECK(!diagonal || dist0 == 0, PHMRF_ERR_INVALID, "a diagonal block has dist0 == 0");
  PHMRF_CHECK(d_min >= 0, PHMRF_ERR_INVALID, "d_min must be >= 0");
  PHMRF_CHECK(d_max == -1 || d_max >= d_min, PHMRF_ERR_INVALID, "d_max must be >= d_min, or -1 for no upper limit");
  PHMRF_CHECK(K <= 64, PHMRF_ERR_UNSUPPORTED, "K must be <= 64");
  PHMRF_CHECK(C <= ENRICH_MAX_CLASSES, PHMRF_ERR_UNSUPPORTED, "C must be <= 8");
  const int64_t n = grid_row_first<int64_t>(H, W, diagonal);
  PHMRF_TRY(check_nodes(n, "n must be below 2^31 - 64"));
  PHMRF_CHECK(dist0 > -((int64_t)1 << 31) && dist0 < ((int64_t)1 << 31) &&
                  (dist0 < 0 ? -dist0 : dist0) + H + W < ((int64_t)1 << 31),
              PHMRF_ERR_UNSUPPORTED, "|dist0| + H + W must be below 2^31");
  const int P = 2 * C * C;
  PHMRF_CHECK(D < ((int64_t)1 << 31) && D * (K > P ? K : P) < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED,
              "D max(K, 2 C C) must be below 2^31");
  // the signed diagonals x = dist0 + j - i of the region, and of them the ones inside the window: xa .. xa + na - 1 >= 0 and
  // xb .. xb + nb - 1 < 0.  Every distance is below INT_MAX: a d_min up there leaves nothing inside, a d_max up there is no limit.
  const int64_t w_lo = d_min < INT_MAX ? d_min : INT_MAX, w_hi = (d_max == -1 || d_max > INT_MAX) ? INT_MAX : d_max;
  const int64_t x_lo = diagonal ? 0 : dist0 - (H - 1), x_hi = diagonal ? H - 1 : dist0 + (W - 1);
  const int64_t xa = x_lo > w_lo ? x_lo : w_lo, xa_end = x_hi < w_hi ? x_hi : w_hi;
  const int64_t xb = x_lo > -w_hi ? x_lo : -w_hi, xb_end = x_hi < -(w_lo > 1 ? w_lo : 1) ? x_hi : -(w_lo > 1 ? w_lo : 1);
  const int64_t na = xa_end >= xa ? xa_end - xa + 1 : 0, nb = xb_end >= xb ? xb_end - xb + 1 : 0;
  if (na + nb > 0) {                                   // the distances inside the window: one range, the table must hold it
    int64_t lo = INT64_MAX, hi = -1;
    if (na) lo = xa, hi = xa_end;
    if (nb) lo = -xb_end < lo ? -xb_end : lo, hi = -xb > hi ? -xb : hi;
    PHMRF_CHECK(d_lo <= lo && hi < d_lo + D, PHMRF_ERR_INVALID, "the table [d_lo, d_lo + D) does not hold every distance inside the window");
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const size_t n_obs = (size_t)P * K, n_sd = (size_t)D * K, n_cd = (size_t)D * P;
  if (na + nb == 0) {                                  // nothing inside the window
    for (size_t t = 0; t < n_obs; ++t) obs_host[t] = 0;
    for (size_t t = 0; t < n_sd; ++t) state_dist_host[t] = 0;
    for (size_t t = 0; t < n_cd; ++t) cat_dist_host[t] = 0;
    return PHMRF_OK;
  }
  const uint8_t* const col_class = diagonal ? row_class_dev : col_class_dev_or_null;
  const int32_t* const col_seg = diagonal ? row_seg_dev_or_null : col_seg_dev_or_null;
  const int per_row = (W + ENRICH_TILE_W - 1) / ENRICH_TILE_W;
  const int64_t ntiles = diagonal ? (int64_t)ENRICH_PER_SUPER * grid_row_first<int64_t>(per_row, per_row, 1)
                                  : (int64_t)((H + ENRICH_TILE_H - 1) / ENRICH_TILE_H) * per_row;
  const int slots = ((H < W ? H : W) + ENRICH_CHUNK - 1) / ENRICH_CHUNK;
  const int64_t nitems = (na + nb) * slots;

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
                     H, W, diagonal, (int)dist0, K, C, row_class_dev, col_class, row_seg_dev_or_null, col_seg, (int)w_lo, (int)w_hi,
                     (int)d_lo, per_row, ntiles, all, state_dist, flag);
  PHMRF_HIP(hipGetLastError());
  hipLaunchKernelGGL(enrich_class_kernel, dim3(grid_of(nitems, 4, ENRICH_GRID_CAP)), dim3(256), 0, st, H, W, diagonal, (int)dist0, C,
                     row_class_dev, col_class, row_seg_dev_or_null, col_seg, (int)xa, (int)na, (int)xb, slots, nitems, (int)d_lo,
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
