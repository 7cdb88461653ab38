// gfx950 kernels of the enrichment's permutation null (phmrf_pair_enrichment_null): ONE region's bin
// pairs counted against T circular shifts of its chromosome's annotation, and per shift the distance-matched expectation in
// 2^-24 fixed point.  Integer arithmetic throughout: no result depends on the order in which the atomics land.
//
//   counting     obs[t][p][k] over the stored nodes INSIDE the distance window.  enrich.hip's tile geometry (a tile of
//                ENRICH_TILE_H storage rows by ENRICH_TILE_W storage columns, a half-wave per row: enrich_tiles.h; label_row, window_tile,
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

#include "enrich_tiles.h"

namespace phmrf {
namespace {

constexpr int NULL_GRID_CAP = 1024;      // workgroups of the counting kernel (enrich.py NULL_GRID_CAP)
constexpr int NULL_CLASS_CAP = 4096;     // workgroups of the expectation kernel (enrich.py NULL_CLASS_CAP)
constexpr int NULL_BINS = ENRICH_TILE_H + ENRICH_TILE_W;       // bins of a tile whose (class, segment) is staged per shift
constexpr int NULL_CHUNK = 512;          // cells of a diagonal a wave of the expectation kernel takes at a time
constexpr int NULL_LDS_BYTES = 65536;    // LDS of the counting kernel (enrich.py NULL_LDS_BYTES)
constexpr int NULL_MAX_GROUP = 16;       // shifts of a group at most (enrich.py NULL_MAX_GROUP)
constexpr int NULL_ACC_BYTES = 49152;    // the expectation kernel's u64 [P][Kc] table at most
constexpr int NULL_MAX_SHIFTS = 4096;
constexpr unsigned NULL_WEIGHT_ONE = 1u << 24;

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
    if (!window_tile<ENRICH_TILE_H, ENRICH_TILE_W>(tile, H, W, diagonal, per_row, dist0, d_lo, d_hi, &t)) continue;
    uint32_t word[ENRICH_PAIRS_PER_WAVE];
    int single[ENRICH_PAIRS_PER_WAVE];
    load_tile_rows<8>(labels, t, W, diagonal, 2 * wave + half, l32, word, single);   // a half-wave per row
    for (int x = threadIdx.x; x < mine_ts * NULL_BINS; x += 256) {
      const int q = x / NULL_BINS, b = x - q * NULL_BINS;
      const unsigned s = (unsigned)shifts[t0 + q];
      const bool column = b < ENRICH_TILE_W;
      const int at = column ? t.j0 + b : t.i0 + (b - ENRICH_TILE_W);
      if (at < (column ? t.j1 : t.i1)) {
        const unsigned g = wrapped((column ? col0 : row0) + (unsigned)at, s, B);
        info[x] = make_int2(cls[g], seg ? seg[g] : -1);
      }
    }
    __syncthreads();                                   // (the first tile: the zeroed tables too)
#pragma unroll
    for (int u = 0; u < ENRICH_PAIRS_PER_WAVE; ++u) {
      if (t.i0 + 2 * wave + 8 * u >= t.i1) break;       // the same for the wave; its second row may still be absent
      const int i = t.i0 + 2 * wave + half + 8 * u;
      const bool present = i < t.i1;
      const LabelRow r = present_row(labels, t, i, present, W, diagonal);
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
      const int j1 = r.ja + r.byte_at(l32) - t.j0;
      if (l32 < r.nvec) {
#pragma unroll
        for (int e = 0; e < 4; ++e) st[e] = state_of((int)((word[u] >> (8 * e)) & 0xff), t.j0 + jv + e);
      }
      if (l32 < r.nbytes) st1 = state_of(single[u], t.j0 + j1);
      const bool bytes = __any(st1 >= 0);
      const int ri = ENRICH_TILE_W + (present ? i - t.i0 : 0);
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
          return pair_bin(mine, other, C) * K + s;
        };
        {
          int key[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) key[e] = st[e] >= 0 ? bin(st[e], jv + e) : -1;
          wave_quad_add(tab, key);
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
// [Kc blockIdx.z, + Kc) below K.  The diagonals and their chunks of NULL_CHUNK rows: diagonal_chunk.
__global__ __launch_bounds__(256) void enrich_null_class_kernel(int H, int W, int diagonal, int dist0, int K, int C,
                                                                const uint8_t* __restrict__ cls, const int32_t* __restrict__ seg,
                                                                unsigned row0, unsigned col0, unsigned B,
                                                                const int32_t* __restrict__ shifts, int xa, int na, int xb, int slots,
                                                                int64_t nitems, int tab_lo, const unsigned* __restrict__ weight, int Kc,
                                                                unsigned long long* __restrict__ expq, int* __restrict__ bad) {
  extern __shared__ unsigned long long null_acc[];    // [P][Kc]
  __shared__ unsigned tabs[4][ENRICH_MAX_PAIRS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* const tab = tabs[wave];
  const int P = 2 * C * C;
  const int k0 = blockIdx.z * Kc, kc = K - k0 < Kc ? K - k0 : Kc;
  const unsigned s = (unsigned)shifts[blockIdx.y];
  for (int q = lane; q < ENRICH_MAX_PAIRS; q += 64) tab[q] = 0;
  for (int x = threadIdx.x; x < P * Kc; x += 256) null_acc[x] = 0;
  __syncthreads();
  bool wrong = false;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < nitems; item += (int64_t)gridDim.x * 4) {
    int x, shift, a, b;
    if (!diagonal_chunk<NULL_CHUNK>(item, slots, xa, na, xb, dist0, H, W, &x, &shift, &a, &b)) continue;
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
          key = pair_bin(make_int2(rc, rs), make_int2(cc, cs), C);
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
  int64_t n;
  PHMRF_TRY(check_region(H, W, diagonal, &n));
  PHMRF_CHECK(K >= 1 && C >= 1, PHMRF_ERR_INVALID, "K and C must be >= 1");
  PHMRF_CHECK(T >= 1, PHMRF_ERR_INVALID, "T must be >= 1");
  PHMRF_CHECK(D >= 0 && d_lo >= 0, PHMRF_ERR_INVALID, "D and d_lo must be >= 0");
  PHMRF_CHECK(!diagonal || row0 == col0, PHMRF_ERR_INVALID, "a diagonal block has row0 == col0");
  PHMRF_CHECK(row0 >= 0 && col0 >= 0 && row0 <= B - H && col0 <= B - W, PHMRF_ERR_INVALID,
              "the region's rows and columns must lie inside the chromosome's B bins");
  PHMRF_TRY(check_window(d_min, d_max));
  PHMRF_TRY(check_states(K));                          // (its upper limit)
  PHMRF_CHECK(C <= ENRICH_MAX_CLASSES, PHMRF_ERR_UNSUPPORTED, "C must be <= 8");
  PHMRF_CHECK(T <= NULL_MAX_SHIFTS, PHMRF_ERR_UNSUPPORTED, "T must be <= 4096");
  const int P = 2 * C * C;
  PHMRF_CHECK((int64_t)T * P * K < ((int64_t)1 << 26), PHMRF_ERR_UNSUPPORTED, "T 2 C C K must be below 2^26");
  PHMRF_CHECK(B < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED, "B must be below 2^31");
  PHMRF_TRY(check_nodes(n, "n must be below 2^31 - 64"));
  const int64_t dist0 = col0 - row0;                   // (|dist0| + H + W < 2 B + ... : B < 2^31 does not bound it)
  PHMRF_TRY(check_span(dist0, H, W));
  PHMRF_CHECK(D < ((int64_t)1 << 31) && D * (K > P ? K : P) < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED,
              "D max(K, 2 C C) must be below 2^31");
  for (int t = 0; t < T; ++t)
    PHMRF_CHECK(shifts_host[t] >= 0 && shifts_host[t] < B, PHMRF_ERR_INVALID, "a shift lies outside 0 .. B - 1");
  const size_t n_w = (size_t)D * K;
  for (size_t t = 0; t < n_w; ++t) PHMRF_CHECK(weight_host[t] <= NULL_WEIGHT_ONE, PHMRF_ERR_INVALID, "a weight is above 2^24");
  // the signed diagonals inside the window and the table's range: as phmrf_pair_enrichment
  const IntWindow win = int_window(d_min, d_max);
  WindowDiagonals dg;
  PHMRF_TRY(window_diagonals(H, W, diagonal, dist0, win, d_lo, D, &dg));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const size_t n_tab = (size_t)T * P * K;
  if (dg.na + dg.nb == 0) {                            // nothing inside the window
    for (size_t t = 0; t < n_tab; ++t) obs_host[t] = expq_host[t] = 0;
    return PHMRF_OK;
  }
  int per_row;
  const int64_t ntiles = window_tile_count<ENRICH_TILE_H, ENRICH_TILE_W>(H, W, diagonal, &per_row);
  const int slots = ((H < W ? H : W) + NULL_CHUNK - 1) / NULL_CHUNK;
  const int64_t nitems = ((int64_t)dg.na + dg.nb) * slots;
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
                     chrom_seg_dev_or_null, (unsigned)row0, (unsigned)col0, (unsigned)B, shifts, T, ts, win.lo, win.hi, per_row,
                     ntiles, all, flag);
  PHMRF_HIP(hipGetLastError());
  const int per_shift = NULL_CLASS_CAP / T > 1 ? NULL_CLASS_CAP / T : 1;
  hipLaunchKernelGGL(enrich_null_class_kernel, dim3(grid_of(nitems, 4, per_shift), T, splits), dim3(256), (size_t)8 * P * Kc, st, H, W,
                     diagonal, (int)dist0, K, C, chrom_class_dev, chrom_seg_dev_or_null, (unsigned)row0, (unsigned)col0, (unsigned)B,
                     shifts, dg.xa, dg.na, dg.xb, slots, nitems, (int)d_lo, weight, Kc, expq, flag);
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
