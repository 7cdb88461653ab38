// gfx950 kernels of the enrichment's permutation null (phmrf_pair_enrichment_null): ONE region's bin
// pairs counted against T circular shifts of its chromosome's annotation, and per shift the distance-matched expectation in
// 2^-24 fixed point.  Integer arithmetic throughout: no result depends on the order in which the atomics land.
//
//   counting     obs[t][p][k] over the stored nodes INSIDE the distance window.  enrich.hip's tile geometry (a tile of
//                ENRICH_TILE_H storage rows by ENRICH_TILE_W storage columns, a half-wave per row: label_row, window_tile,
//                wave_run_add of runs.h).  A workgroup owns a GROUP of up to TS shifts (blockIdx.y; null_group_shifts: as many
//                as fit the 64 KB of LDS a launch gets without asking, at most NULL_MAX_GROUP) and strides over the tiles:
//                a tile's labels are loaded ONCE into registers and counted against every shift of the group.  Per tile the
//                (class, segment) of its 160 bins under every shift of the group is staged in LDS, 8 bytes a bin, from
//                chrom_class[(row0 + i + s) mod B]: the wrap seam may fall anywhere in the tile's rows or columns.  The group's
//                TS tables u32 [P][K] live in LDS for the workgroup's life and are flushed once with u64 global atomics on the
//                non-zero bins.  The state map does not move, so there is no distance table here.
//   expectation  expq[t][p][k] = sum_d cat_t[d][p] w[d][k], fused: cat_t is never stored.  enrich_class_kernel's walk along the
//                signed diagonals with the shift as one more index (blockIdx.y): a wave takes NULL_CHUNK consecutive rows of
//                ONE signed diagonal, wave_run_add into its own [P] table in LDS, then lane k adds count * w[d][k] for the few
//                non-zero p to the workgroup's u64 [P][Kc] table in LDS (LDS atomics; Kc <= K states per workgroup so that the
//                table stays within NULL_ACC_BYTES, blockIdx.z the slice).  The table goes to expq once, when the workgroup is
//                done, with u64 global atomics on the non-zero entries: no global atomic per wave-chunk at all.
//                count < 2^31 and w <= 2^24: a region's sums stay below 2^55.
//   A label >= K inside the window sets bit 0 of the flag word, a class >= C on a node inside the window under one of the
//   call's shifts bit 1; nodes outside the window are not inspected.

#include "runs.h"

#include <climits>

namespace phmrf {
namespace {

constexpr int NULL_GRID_CAP = 1024;      // workgroups of the counting kernel (enrich.py NULL_GRID_CAP)
constexpr int NULL_CLASS_CAP = 4096;     // workgroups of the expectation kernel (enrich.py NULL_CLASS_CAP)
constexpr int NULL_TILE_H = 32;          // enrich.hip's tile: storage rows ...
constexpr int NULL_TILE_W = 128;         // ... and storage columns, 32 lanes x 4 labels
constexpr int NULL_BINS = NULL_TILE_H + NULL_TILE_W;           // bins of a tile whose (class, segment) is staged per shift
constexpr int NULL_PAIRS_PER_WAVE = NULL_TILE_H / 8;           // a workgroup is four waves of two rows each
constexpr int NULL_PER_SUPER = NULL_TILE_W / NULL_TILE_H;      // tiles of a square super-tile (diagonal blocks)
constexpr int NULL_CHUNK = 512;          // cells of a diagonal a wave of the expectation kernel takes at a time
constexpr int NULL_MAX_CLASSES = 8;
constexpr int NULL_MAX_PAIRS = 2 * NULL_MAX_CLASSES * NULL_MAX_CLASSES;
constexpr int NULL_LDS_BYTES = 65536;    // LDS of the counting kernel (enrich.py NULL_LDS_BYTES)
constexpr int NULL_MAX_GROUP = 16;       // shifts of a group at most (enrich.py NULL_MAX_GROUP)
constexpr int NULL_ACC_BYTES = 49152;    // the expectation kernel's u64 [P][Kc] table at most
constexpr int NULL_MAX_SHIFTS = 4096;
constexpr unsigned NULL_WEIGHT_ONE = 1u << 24;
constexpr int BAD_LABEL = 1, BAD_CLASS = 2;

// shifts of a group (enrich.py null_group): a count table of u32 [2 C C][K] and 8 bytes for each of the tile's bins per shift
inline int null_group_shifts(int K, int C) {
  const int per = 4 * 2 * C * C * K + 8 * NULL_BINS;
  const int ts = NULL_LDS_BYTES / per;
  return ts < 1 ? 1 : (ts > NULL_MAX_GROUP ? NULL_MAX_GROUP : ts);
}

// bin (at + s) mod B for at < B and s < B < 2^31
__device__ __forceinline__ unsigned wrapped(unsigned at, unsigned s, unsigned B) {
  const unsigned g = at + s;
  return g >= B ? g - B : g;
}

// obs: u64 [T][2 C C][K]; the group blockIdx.y holds the shifts [ts blockIdx.y, ts blockIdx.y + ts) below T.  d_hi: INT_MAX
// for no upper limit.  cls / seg: the chromosome's [B] arrays, seg null without segments.
__global__ __launch_bounds__(256) void enrich_null_label_kernel(const uint8_t* __restrict__ labels, int H, int W, int diagonal, int dist0,
                                                                int K, int C, const uint8_t* __restrict__ cls,
                                                                const int32_t* __restrict__ seg, unsigned row0, unsigned col0,
                                                                unsigned B, const int32_t* __restrict__ shifts, int T, int ts,
                                                                int d_lo, int d_hi, int per_row, int64_t ntiles,
                                                                unsigned long long* __restrict__ obs, int* __restrict__ bad) {
  extern __shared__ int2 null_lds[];
  int2* const info = null_lds;                                         // [ts][NULL_BINS]: the tile's columns, then its rows
  unsigned* const tabs = reinterpret_cast<unsigned*>(null_lds + ts * NULL_BINS);   // [ts][nobs]
  const int nobs = 2 * C * C * K;
  const int t0 = blockIdx.y * ts, mine_ts = T - t0 < ts ? T - t0 : ts;
  for (int x = threadIdx.x; x < mine_ts * nobs; x += 256) tabs[x] = 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l32 = lane & 31;
  int wrong = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    WindowTile t;
    if (!window_tile<NULL_TILE_H, NULL_TILE_W>(tile, H, W, diagonal, per_row, dist0, d_lo, d_hi, &t)) continue;
    // the half-wave's rows i0 + 2 wave + half, + 8, ...: every load of the tile is issued before the first count
    uint32_t word[NULL_PAIRS_PER_WAVE];
    int single[NULL_PAIRS_PER_WAVE];
#pragma unroll
    for (int u = 0; u < NULL_PAIRS_PER_WAVE; ++u) {
      const int i = t.i0 + 2 * wave + half + 8 * u;
      word[u] = 0;
      single[u] = 0;
      if (i < t.i1) {
        const LabelRow r = label_row(labels, i, t.j0, t.j1, W, diagonal);
        if (l32 < r.nvec) word[u] = *reinterpret_cast<const uint32_t*>(r.p + r.head + 4 * l32);
        if (l32 < r.nbytes) single[u] = r.p[l32 < r.head ? l32 : r.tail + (l32 - r.head)];
      }
    }
    for (int x = threadIdx.x; x < mine_ts * NULL_BINS; x += 256) {
      const int q = x / NULL_BINS, b = x - q * NULL_BINS;
      const unsigned s = (unsigned)shifts[t0 + q];
      const bool column = b < NULL_TILE_W;
      const int at = column ? t.j0 + b : t.i0 + (b - NULL_TILE_W);
      if (at < (column ? t.j1 : t.i1)) {
        const unsigned g = wrapped((column ? col0 : row0) + (unsigned)at, s, B);
        info[x] = make_int2(cls[g], seg ? seg[g] : -1);
      }
    }
    __syncthreads();                                   // (the first tile: the zeroed tables too)
#pragma unroll
    for (int u = 0; u < NULL_PAIRS_PER_WAVE; ++u) {
      if (t.i0 + 2 * wave + 8 * u >= t.i1) break;       // the same for the wave; its second row may still be absent
      const int i = t.i0 + 2 * wave + half + 8 * u;
      const bool present = i < t.i1;
      LabelRow r = label_row(labels, present ? i : t.i0, t.j0, t.j1, W, diagonal);
      if (!present) r.nvec = r.nbytes = 0;
      const int x0 = dist0 - i;                         // the cell's distance is |x0 + j|
      // one cell, whatever the shift: its state, -1 outside the window or with a label >= K
      auto state_of = [&](int s, int j) -> int {
        const int x = x0 + j, d = x < 0 ? -x : x;
        if (!t.whole && (d < d_lo || d > d_hi)) return -1;
        if (s >= K) {
          wrong |= BAD_LABEL;
          return -1;
        }
        return s;
      };
      int st[4] = {-1, -1, -1, -1}, st1 = -1;
      const int jv = r.ja + r.head + 4 * l32 - t.j0;    // the lane's first word column, from the tile's first
      const int j1 = r.ja + (l32 < r.head ? l32 : r.tail + (l32 - r.head)) - t.j0;
      if (l32 < r.nvec) {
#pragma unroll
        for (int e = 0; e < 4; ++e) st[e] = state_of((int)((word[u] >> (8 * e)) & 0xff), t.j0 + jv + e);
      }
      if (l32 < r.nbytes) st1 = state_of(single[u], t.j0 + j1);
      const bool bytes = __any(st1 >= 0);
      const int ri = NULL_TILE_W + (present ? i - t.i0 : 0);
      for (int q = 0; q < mine_ts; ++q) {
        const int2* const inf = info + q * NULL_BINS;
        unsigned* const tab = tabs + q * nobs;
        const int2 mine = inf[ri];
        // the obs bin of a cell in state s >= 0 at the tile's column c; -1 with a class >= C
        auto bin = [&](int s, int c) -> int {
          const int2 other = inf[c];
          if (mine.x >= C || other.x >= C) {
            wrong |= BAD_CLASS;
            return -1;
          }
          const int same = (mine.y >= 0 && mine.y == other.y) ? 1 : 0;
          return ((mine.x * C + other.x) * 2 + same) * K + s;
        };
        {
          int key[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) key[e] = st[e] >= 0 ? bin(st[e], jv + e) : -1;
          unsigned lead = key[0] >= 0 ? 1u : 0u;        // the lane's cells in the bin of its first
          int e = 1;
          for (; e < 4 && lead && key[e] == key[0]; ++e) ++lead;
          wave_run_add(tab, key[0], lead);
          for (; e < 4; ++e)
            if (key[e] >= 0) atomicAdd(tab + key[e], 1u);
        }
        if (bytes) {                                    // (the same for the wave)
          const int key = st1 >= 0 ? bin(st1, j1) : -1;
          wave_run_add(tab, key, key >= 0 ? 1u : 0u);
        }
      }
    }
    __syncthreads();                                   // the next tile's staging overwrites the bins
  }
  __syncthreads();                                     // (a workgroup without a tile: the zeroed tables)
  for (int x = threadIdx.x; x < mine_ts * nobs; x += 256) {
    const unsigned c = tabs[x];
    if (c) atomicAdd(obs + (size_t)t0 * nobs + x, (unsigned long long)c);
  }
  if (wrong) atomicOr(bad, wrong);
}

// expq: u64 [T][2 C C][K]; weight: u32 [D][K], row 0 the distance tab_lo.  blockIdx.y: the shift; blockIdx.z: the states
// [Kc blockIdx.z, + Kc) below K.  The diagonals: x = xa + t for t < na, x = xb + (t - na) for the nb after them; `slots` chunks
// of NULL_CHUNK rows cover the longest diagonal; item = t slots + slot.
__global__ __launch_bounds__(256) void enrich_null_class_kernel(int H, int W, int diagonal, int dist0, int K, int C,
                                                                const uint8_t* __restrict__ cls, const int32_t* __restrict__ seg,
                                                                unsigned row0, unsigned col0, unsigned B,
                                                                const int32_t* __restrict__ shifts, int xa, int na, int xb, int slots,
                                                                int64_t nitems, int tab_lo, const unsigned* __restrict__ weight, int Kc,
                                                                unsigned long long* __restrict__ expq, int* __restrict__ bad) {
  extern __shared__ unsigned long long null_acc[];    // [P][Kc]
  __shared__ unsigned tabs[4][NULL_MAX_PAIRS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* const tab = tabs[wave];
  const int P = 2 * C * C;
  const int k0 = blockIdx.z * Kc, kc = K - k0 < Kc ? K - k0 : Kc;
  const unsigned s = (unsigned)shifts[blockIdx.y];
  for (int q = lane; q < NULL_MAX_PAIRS; q += 64) tab[q] = 0;
  for (int x = threadIdx.x; x < P * Kc; x += 256) null_acc[x] = 0;
  __syncthreads();
  bool wrong = false;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < nitems; item += (int64_t)gridDim.x * 4) {
    const int t = (int)(item / slots), slot = (int)(item - (int64_t)t * slots);
    const int x = t < na ? xa + t : xb + (t - na);
    // the rows i of the diagonal: 0 <= i < H and 0 <= j = i + x - dist0 < W
    const int shift = x - dist0;                        // in [-(H - 1), W - 1]
    const int i_lo = shift < 0 ? -shift : 0, i_hi = W - shift < H ? W - shift : H;
    const int64_t a64 = (int64_t)i_lo + (int64_t)slot * NULL_CHUNK;
    if (a64 >= i_hi) continue;                          // (the same for the wave)
    const int a = (int)a64, b = i_hi - a > NULL_CHUNK ? a + NULL_CHUNK : i_hi;
    for (int base = a; base < b; base += 64) {
      const int i = base + lane;
      int key = -1;
      if (i < b) {
        const unsigned gi = wrapped(row0 + (unsigned)i, s, B), gj = wrapped(col0 + (unsigned)(i + shift), s, B);
        const int rc = cls[gi], cc = cls[gj];
        if (rc >= C || cc >= C) {
          wrong = true;
        } else {
          const int rs = seg ? seg[gi] : -1, cs = seg ? seg[gj] : -1;
          key = (rc * C + cc) * 2 + ((rs >= 0 && rs == cs) ? 1 : 0);
        }
      }
      wave_run_add(tab, key, key >= 0 ? 1u : 0u);
    }
    const int d = x < 0 ? -x : x;
    const unsigned long long wk = lane < kc ? weight[(size_t)(d - tab_lo) * K + k0 + lane] : 0u;
    for (int q0 = 0; q0 < P; q0 += 64) {                // (LDS operations of one wave complete in order)
      unsigned c = 0;
      if (q0 + lane < P) {
        c = tab[q0 + lane];
        if (c) tab[q0 + lane] = 0;
      }
      unsigned long long held = __ballot(c != 0);
      while (held) {                                    // the few categories of the chunk, lane <-> state
        const int from = __ffsll((long long)held) - 1;
        held &= held - 1;
        const unsigned long long count = (unsigned)__shfl((int)c, from, 64);
        if (wk) atomicAdd(null_acc + (q0 + from) * Kc + lane, count * wk);
      }
    }
  }
  __syncthreads();
  for (int x = threadIdx.x; x < P * Kc; x += 256) {
    const unsigned long long c = null_acc[x];
    const int p = x / Kc, k = x - p * Kc;
    if (c && k < kc) atomicAdd(expq + ((size_t)blockIdx.y * P + p) * K + k0 + k, c);
  }
  if (wrong) atomicOr(bad, BAD_CLASS);
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_pair_enrichment_null(const uint8_t* labels_dev, int H, int W, int diagonal, int64_t row0, int64_t col0, int K, int C,
                               const uint8_t* chrom_class_dev, const int32_t* chrom_seg_dev_or_null, int64_t B,
                               const int32_t* shifts_host, int T, int64_t d_min, int64_t d_max, int64_t d_lo, int64_t D,
                               const uint32_t* weight_host, int64_t* obs_host, int64_t* expq_host, void* hip_stream) {
  PHMRF_CHECK(labels_dev && chrom_class_dev && shifts_host && weight_host && obs_host && expq_host, PHMRF_ERR_INVALID,
              "NULL labels, classes, shifts, weights or output table");
  PHMRF_CHECK(diagonal == 0 || diagonal == 1, PHMRF_ERR_INVALID, "diagonal must be 0 or 1");
  PHMRF_CHECK(H >= 1 && W >= 1, PHMRF_ERR_INVALID, "H and W must be >= 1");
  PHMRF_CHECK(K >= 1 && C >= 1, PHMRF_ERR_INVALID, "K and C must be >= 1");
  PHMRF_CHECK(T >= 1, PHMRF_ERR_INVALID, "T must be >= 1");
  PHMRF_CHECK(D >= 0 && d_lo >= 0, PHMRF_ERR_INVALID, "D and d_lo must be >= 0");
  PHMRF_CHECK(!diagonal || H == W, PHMRF_ERR_INVALID, "a diagonal block is square (H == W)");
  PHMRF_CHECK(!diagonal || row0 == col0, PHMRF_ERR_INVALID, "a diagonal block has row0 == col0");
  PHMRF_CHECK(row0 >= 0 && col0 >= 0 && row0 <= B - H && col0 <= B - W, PHMRF_ERR_INVALID,
              "the region's rows and columns must lie inside the chromosome's B bins");
  PHMRF_CHECK(d_min >= 0, PHMRF_ERR_INVALID, "d_min must be >= 0");
  PHMRF_CHECK(d_max == -1 || d_max >= d_min, PHMRF_ERR_INVALID, "d_max must be >= d_min, or -1 for no upper limit");
  PHMRF_CHECK(K <= 64, PHMRF_ERR_UNSUPPORTED, "K must be <= 64");
  PHMRF_CHECK(C <= NULL_MAX_CLASSES, PHMRF_ERR_UNSUPPORTED, "C must be <= 8");
  PHMRF_CHECK(T <= NULL_MAX_SHIFTS, PHMRF_ERR_UNSUPPORTED, "T must be <= 4096");
  const int P = 2 * C * C;
  PHMRF_CHECK((int64_t)T * P * K < ((int64_t)1 << 26), PHMRF_ERR_UNSUPPORTED, "T 2 C C K must be below 2^26");
  PHMRF_CHECK(B < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED, "B must be below 2^31");
  const int64_t n = grid_row_first<int64_t>(H, W, diagonal);
  PHMRF_TRY(check_nodes(n, "n must be below 2^31 - 64"));
  const int64_t dist0 = col0 - row0;                   // (|dist0| + H + W < 2 B + ... : B < 2^31 does not bound it)
  PHMRF_CHECK((dist0 < 0 ? -dist0 : dist0) + H + W < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED, "|dist0| + H + W must be below 2^31");
  PHMRF_CHECK(D < ((int64_t)1 << 31) && D * (K > P ? K : P) < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED,
              "D max(K, 2 C C) must be below 2^31");
  for (int t = 0; t < T; ++t)
    PHMRF_CHECK(shifts_host[t] >= 0 && shifts_host[t] < B, PHMRF_ERR_INVALID, "a shift lies outside 0 .. B - 1");
  const size_t n_w = (size_t)D * K;
  for (size_t t = 0; t < n_w; ++t) PHMRF_CHECK(weight_host[t] <= NULL_WEIGHT_ONE, PHMRF_ERR_INVALID, "a weight is above 2^24");
  // the signed diagonals inside the window and the table's range: as phmrf_pair_enrichment
  const int64_t w_lo = d_min < INT_MAX ? d_min : INT_MAX, w_hi = (d_max == -1 || d_max > INT_MAX) ? INT_MAX : d_max;
  const int64_t x_lo = diagonal ? 0 : dist0 - (H - 1), x_hi = diagonal ? H - 1 : dist0 + (W - 1);
  const int64_t xa = x_lo > w_lo ? x_lo : w_lo, xa_end = x_hi < w_hi ? x_hi : w_hi;
  const int64_t xb = x_lo > -w_hi ? x_lo : -w_hi, xb_end = x_hi < -(w_lo > 1 ? w_lo : 1) ? x_hi : -(w_lo > 1 ? w_lo : 1);
  const int64_t na = xa_end >= xa ? xa_end - xa + 1 : 0, nb = xb_end >= xb ? xb_end - xb + 1 : 0;
  if (na + nb > 0) {
    int64_t lo = INT64_MAX, hi = -1;
    if (na) lo = xa, hi = xa_end;
    if (nb) lo = -xb_end < lo ? -xb_end : lo, hi = -xb > hi ? -xb : hi;
    PHMRF_CHECK(d_lo <= lo && hi < d_lo + D, PHMRF_ERR_INVALID, "the table [d_lo, d_lo + D) does not hold every distance inside the window");
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const size_t n_tab = (size_t)T * P * K;
  if (na + nb == 0) {                                  // nothing inside the window
    for (size_t t = 0; t < n_tab; ++t) obs_host[t] = expq_host[t] = 0;
    return PHMRF_OK;
  }
  const int per_row = (W + NULL_TILE_W - 1) / NULL_TILE_W;
  const int64_t ntiles = diagonal ? (int64_t)NULL_PER_SUPER * grid_row_first<int64_t>(per_row, per_row, 1)
                                  : (int64_t)((H + NULL_TILE_H - 1) / NULL_TILE_H) * per_row;
  const int slots = ((H < W ? H : W) + NULL_CHUNK - 1) / NULL_CHUNK;
  const int64_t nitems = (na + nb) * slots;
  const int ts = null_group_shifts(K, C), groups = (T + ts - 1) / ts;
  const int splits = (8 * P * K + NULL_ACC_BYTES - 1) / NULL_ACC_BYTES, Kc = (K + splits - 1) / splits;

  // one allocation and one memset: obs u64 [T P K] | expq u64 [T P K] | the flag word || weights u32 [D K] | shifts i32 [T]
  Buffers buf;
  unsigned long long* all;
  const size_t n_zero = 2 * n_tab + 1;
  PHMRF_TRY(buf.get(&all, n_zero + (n_w + (size_t)T + 1) / 2));
  unsigned long long* const expq = all + n_tab;
  int* const flag = reinterpret_cast<int*>(all + 2 * n_tab);
  unsigned* const weight = reinterpret_cast<unsigned*>(all + n_zero);
  int32_t* const shifts = reinterpret_cast<int32_t*>(weight + n_w);
  PHMRF_HIP(hipMemsetAsync(all, 0, n_zero * sizeof(unsigned long long), st));
  if (n_w) PHMRF_HIP(hipMemcpyAsync(weight, weight_host, n_w * sizeof(unsigned), hipMemcpyHostToDevice, st));
  PHMRF_HIP(hipMemcpyAsync(shifts, shifts_host, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice, st));
  const int per_group = NULL_GRID_CAP / groups > 1 ? NULL_GRID_CAP / groups : 1;
  hipLaunchKernelGGL(enrich_null_label_kernel, dim3(grid_of(ntiles, 1, per_group), groups), dim3(256),
                     (size_t)ts * (8 * NULL_BINS + 4 * (size_t)P * K), st, labels_dev, H, W, diagonal, (int)dist0, K, C, chrom_class_dev,
                     chrom_seg_dev_or_null, (unsigned)row0, (unsigned)col0, (unsigned)B, shifts, T, ts, (int)w_lo, (int)w_hi, per_row,
                     ntiles, all, flag);
  PHMRF_HIP(hipGetLastError());
  const int per_shift = NULL_CLASS_CAP / T > 1 ? NULL_CLASS_CAP / T : 1;
  hipLaunchKernelGGL(enrich_null_class_kernel, dim3(grid_of(nitems, 4, per_shift), T, splits), dim3(256), (size_t)8 * P * Kc, st, H, W,
                     diagonal, (int)dist0, K, C, chrom_class_dev, chrom_seg_dev_or_null, (unsigned)row0, (unsigned)col0, (unsigned)B,
                     shifts, (int)xa, (int)na, (int)xb, slots, nitems, (int)d_lo, weight, Kc, expq, flag);
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  PHMRF_CHECK(!(bad & BAD_LABEL), PHMRF_ERR_INVALID, "a label inside the window is >= K");
  PHMRF_CHECK(!(bad & BAD_CLASS), PHMRF_ERR_INVALID, "a class of a node inside the window under one of the shifts is >= C");
  // unsigned counts below 2^63: the same bytes as int64
  PHMRF_HIP(hipMemcpyAsync(obs_host, all, n_tab * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipMemcpyAsync(expq_host, expq, n_tab * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  return PHMRF_OK;
}

}  // extern "C"
