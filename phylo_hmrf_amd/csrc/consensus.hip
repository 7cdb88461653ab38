// gfx950 kernels of the consensus of M state maps of one region (phmrf_label_consensus).  Integer
// arithmetic throughout: no result depends on the order in which the atomics land.
//
//   check      every map on its own (grid.y = the map): a raw label >= 64, or one whose renumbered state is 255 or >= K.
//              Nothing is written before this pass has found the maps clean.
//   vote       a workgroup takes CONS_PER_TRIP consecutive nodes per grid-stride trip.  STAGE: every map's slice goes into an
//              LDS tile in node order, renumbered on the way: one 4-byte load per lane where the map's own address is
//              aligned, its (at most three) head and tail bytes singly -- a map's alignment is nobody else's business.
//              VOTE: a lane takes four nodes; per node the maps' one-hot 64-bit masks are added into five bit-sliced count
//              planes, the maximum is read off plane by plane from the top and __ffsll gives the lowest tied state.  TABLES:
//              support_hist, agree and bands in LDS, one atomic per run of equal key among consecutive lanes (wave_run_add)
//              for the run that starts a lane's four, the rest singly.  PAIR: a lane owns one pair of maps and a share of the
//              tile, compares sixteen nodes per step and keeps its count in a register until the end.  The tables are
//              flushed once, with one u64 global atomic per non-zero bin.
//   agree      M K K bins do not fit a workgroup (256 KB at M = 16, K = 64): the vote kernel takes the first maps that fit
//              CONS_AGREE_BINS, consensus_agree_kernel the others, chunk by chunk, over the consensus plane just written.

#include "runs.h"

namespace phmrf {
namespace {

constexpr int CONS_GRID_CAP = 1024;      // workgroups of the vote kernel (consensus.py CONSENSUS_GRID_CAP)
constexpr int CONS_PER_TRIP = 1024;      // nodes a workgroup takes per grid-stride trip: 256 lanes x 4 nodes
constexpr int CONS_AGREE_BINS = 8192;    // u32 bins of agree a workgroup holds at a time (32 KB)
constexpr int CONS_VOID = 0x80;          // tile byte of a node past the region's end: | the map, so that no two are equal

struct ConsensusMaps {
  const uint8_t* p[PHMRF_CONSENSUS_MAPS];
  uint8_t ren[PHMRF_CONSENSUS_MAPS][64];
  unsigned long long allowed[PHMRF_CONSENSUS_MAPS];    // bit l: raw label l renumbers to a state < K
};

// bad |= 1 for a raw label >= 64, 2 for one that is not a state of its map or renumbers to >= K
__global__ __launch_bounds__(256) void consensus_check_kernel(ConsensusMaps maps, int64_t n, int* __restrict__ bad) {
  const int m = blockIdx.y;
  const uint8_t* __restrict__ a = maps.p[m];
  const unsigned long long allowed = maps.allowed[m];
  int64_t head = (int64_t)((4 - (reinterpret_cast<uintptr_t>(a) & 3)) & 3);
  if (head > n) head = n;
  const int64_t nvec = (n - head) / 4, tail = head + 4 * nvec, nbytes = head + (n - tail);
  const uint32_t* __restrict__ a4 = reinterpret_cast<const uint32_t*>(a + head);
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  int wrong = 0;
  for (int64_t u = first; u < nvec; u += stride) {
    const uint32_t w = a4[u];
    if (w & 0xc0c0c0c0u) wrong |= 1;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (!((allowed >> ((w >> (8 * e)) & 63)) & 1ull)) wrong |= 2;
  }
  for (int64_t q = first; q < nbytes; q += stride) {
    const int l = a[q < head ? q : tail + (q - head)];
    if (l >= 64) wrong |= 1;
    if (!((allowed >> (l & 63)) & 1ull)) wrong |= 2;
  }
  if (wrong) atomicOr(bad, wrong);
}

// tile[0 .. CONS_PER_TRIP) = the map's nodes [s, s + cnt) through ren (LDS [64]; null: as they are), `fill` past cnt.  One
// aligned 4-byte load per lane and the head and tail bytes of THIS map's address; 256 lanes, all of which call it.
__device__ __forceinline__ void stage_map(uint8_t* tile, const uint8_t* __restrict__ src, int cnt, const uint8_t* ren, int fill) {
  int head = (int)((4 - (reinterpret_cast<uintptr_t>(src) & 3)) & 3);
  if (head > cnt) head = cnt;
  const int nvec = (cnt - head) >> 2, tail = head + 4 * nvec, nbytes = head + (cnt - tail);
  const int t = threadIdx.x;
  if (t < nvec) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(src + head)[t];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int l = (w >> (8 * e)) & 0xff;
      tile[head + 4 * t + e] = ren ? ren[l & 63] : (uint8_t)l;
    }
  }
  if (t < nbytes) {
    const int q = t < head ? t : tail + (t - head);
    const int l = src[q];
    tile[q] = ren ? ren[l & 63] : (uint8_t)l;
  }
  for (int q = cnt + t; q < CONS_PER_TRIP; q += 256) tile[q] = (uint8_t)fill;
}

// floor(sqrt(x)), bit by bit
__device__ __forceinline__ unsigned isqrt64(unsigned long long x) {
  unsigned long long r = 0;
  int sh = x ? (63 - __clzll((long long)x)) & ~1 : 0;
  for (unsigned long long bit = 1ull << sh; bit; bit >>= 2) {
    if (x >= r + bit) {
      x -= r + bit;
      r = (r >> 1) + bit;
    } else {
      r >>= 1;
    }
  }
  return (unsigned)r;
}

// (i, j) of stored node v in integers alone (grid_coords goes through a square root that is not)
__device__ __forceinline__ void int_coords(int64_t v, int W, int diagonal, int* i, int* j) {
  if (!diagonal) {
    const unsigned r = (unsigned)v / (unsigned)W;
    *i = (int)r;
    *j = (int)((unsigned)v - r * (unsigned)W);
    return;
  }
  // the largest r with r W - r (r - 1) / 2 <= v:  r = floor((b - sqrt(b^2 - 8 v)) / 2), b = 2 W + 1, up to the rounding
  const unsigned long long b = 2ull * W + 1ull;
  const unsigned root = isqrt64(b * b - 8ull * (unsigned long long)v);
  int r = (int)(((long long)b - (long long)root) >> 1);
  r = r < 0 ? 0 : (r > W - 1 ? W - 1 : r);
  while (r > 0 && grid_row_first(r, W, 1) > v) --r;
  while (r + 1 < W && grid_row_first(r + 1, W, 1) <= v) ++r;
  *i = r;
  *j = r + (int)(v - grid_row_first(r, W, 1));
}

// 0x80 in every byte of x that is zero
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) {
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// LDS of the vote kernel, in this order: M tiles of CONS_PER_TRIP bytes, M x 64 renumbering bytes, then the u32 tables
// hist [K (M + 1)], pair [M M], bands [32 x 3], agree [am K K] for the maps [0, am)
__global__ __launch_bounds__(256) void consensus_vote_kernel(ConsensusMaps maps, int M, int identity, int K, int64_t n, int W,
                                                             int diagonal, long long dist0, int min_support, int am,
                                                             uint8_t* __restrict__ cons_out, uint8_t* __restrict__ support_out,
                                                             uint8_t* __restrict__ core_out,
                                                             unsigned long long* __restrict__ tables) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint8_t* tiles = lds;
  uint8_t* ren = lds + M * CONS_PER_TRIP;
  unsigned* hist = reinterpret_cast<unsigned*>(ren + M * 64);
  const int n_hist = K * (M + 1), n_pair = M * M, n_bands = PHMRF_DIFF_BANDS * 3, n_agree = am * K * K;
  unsigned* pair = hist + n_hist;
  unsigned* bands = pair + n_pair;
  unsigned* agree = bands + n_bands;
  const int n_bins = n_hist + n_pair + n_bands + n_agree;
  const int tid = threadIdx.x;
  for (int t = tid; t < n_bins; t += 256) hist[t] = 0;
  for (int t = tid; t < M * 64; t += 256) ren[t] = maps.ren[t >> 6][t & 63];

  // the pair of maps (pa, pb) and the share of a tile's 64 steps of sixteen nodes this lane compares
  const int n_pairs = M * (M - 1) / 2;
  const int shares = n_pairs ? (256 / n_pairs < 64 ? 256 / n_pairs : 64) : 0;
  int pa = 0, pb = 0, share = tid / (n_pairs ? n_pairs : 1);
  if (n_pairs && share < shares) {
    int p = tid - share * n_pairs;
    while (p >= M - 1 - pa) {
      p -= M - 1 - pa;
      ++pa;
    }
    pb = pa + 1 + p;
  } else {
    share = -1;
  }
  unsigned pair_count = 0;

  for (int64_t s = (int64_t)blockIdx.x * CONS_PER_TRIP; s < n; s += (int64_t)gridDim.x * CONS_PER_TRIP) {
    const int cnt = n - s < CONS_PER_TRIP ? (int)(n - s) : CONS_PER_TRIP;
    __syncthreads();                                   // (the tiles of the previous trip have been read; the tables are zero)
    for (int m = 0; m < M; ++m)
      stage_map(tiles + m * CONS_PER_TRIP, maps.p[m] + s, cnt, identity ? nullptr : ren + m * 64, CONS_VOID | m);
    __syncthreads();

    // the vote of the lane's four nodes: c[e][p] = bit p of the votes of every state at node e
    unsigned long long c[4][5];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int p = 0; p < 5; ++p) c[e][p] = 0ull;
    for (int m = 0; m < M; ++m) {
      const uint32_t w = reinterpret_cast<const uint32_t*>(tiles + m * CONS_PER_TRIP)[tid];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        unsigned long long carry = 1ull << ((w >> (8 * e)) & 63);
#pragma unroll
        for (int p = 0; p < 5; ++p) {
          const unsigned long long both = c[e][p] & carry;
          c[e][p] ^= carry;
          carry = both;
        }
      }
    }
    const int v0 = 4 * tid;                            // the lane's first node of the trip
    int state[4], sup[4];
    uint32_t cons_w = 0, sup_w = 0, core_w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      unsigned long long cand = ~0ull;
      int votes = 0;
#pragma unroll
      for (int p = 4; p >= 0; --p) {
        const unsigned long long t = cand & c[e][p];
        if (t) {
          cand = t;
          votes |= 1 << p;
        }
      }
      state[e] = v0 + e < cnt ? __ffsll((long long)cand) - 1 : -1;
      sup[e] = votes;
      cons_w |= (uint32_t)(state[e] & 0xff) << (8 * e);
      sup_w |= (uint32_t)votes << (8 * e);
      core_w |= (uint32_t)(votes >= min_support ? state[e] & 0xff : K) << (8 * e);
    }
    // the planes: a word where the plane's address allows and all four nodes exist
    if (v0 < cnt) {
      const int have = cnt - v0 < 4 ? cnt - v0 : 4;
      uint8_t* const outs[3] = {cons_out, support_out, core_out};
      const uint32_t words[3] = {cons_w, sup_w, core_w};
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        if (!outs[o]) continue;
        uint8_t* dst = outs[o] + s + v0;
        if (have == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
          *reinterpret_cast<uint32_t*>(dst) = words[o];
        } else {
          for (int e = 0; e < have; ++e) dst[e] = (uint8_t)(words[o] >> (8 * e));
        }
      }
    }

    // support_hist and the bands
    int key[4], band[4];
    unsigned one[4], stable[4], all[4];
    int i = 0, j = 0;
    if (v0 < cnt) int_coords(s + v0, W, diagonal, &i, &j);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool on = state[e] >= 0;
      key[e] = on ? state[e] * (M + 1) + sup[e] : -1;
      const long long d = dist0 + j - i;
      band[e] = on ? 3 * band_of(d < 0 ? -d : d) : -1;
      one[e] = 1u;
      stable[e] = sup[e] >= min_support ? 1u : 0u;
      all[e] = sup[e] == M ? 1u : 0u;
      if (++j == W) {                                  // the next node starts the next storage row
        ++i;
        j = diagonal ? i : 0;
      }
    }
    wave_quad_add(hist, key, one);
    wave_quad_add(bands, band, one);
    wave_quad_add(bands + 1, band, stable);
    wave_quad_add(bands + 2, band, all);

    // agree of the maps [0, am)
    for (int m = 0; m < am; ++m) {
      const uint32_t w = reinterpret_cast<const uint32_t*>(tiles + m * CONS_PER_TRIP)[tid];
#pragma unroll
      for (int e = 0; e < 4; ++e) key[e] = state[e] >= 0 ? (m * K + state[e]) * K + (int)((w >> (8 * e)) & 63) : -1;
      wave_quad_add(agree, key, one);
    }

    // pair: sixteen nodes of both maps per step
    if (share >= 0) {
      const uint4* ta = reinterpret_cast<const uint4*>(tiles + pa * CONS_PER_TRIP);
      const uint4* tb = reinterpret_cast<const uint4*>(tiles + pb * CONS_PER_TRIP);
      for (int q = share; q < CONS_PER_TRIP / 16 && 16 * q < cnt; q += shares) {
        const uint4 x = ta[q], y = tb[q];
        pair_count += __popc(zero_bytes(x.x ^ y.x)) + __popc(zero_bytes(x.y ^ y.y)) + __popc(zero_bytes(x.z ^ y.z)) +
                      __popc(zero_bytes(x.w ^ y.w));
      }
    }
  }
  if (share >= 0 && pair_count) atomicAdd(pair + pa * M + pb, pair_count);
  __syncthreads();
  // the tables in the order of the device buffer: hist, pair, bands, then agree [M K K], of which [am K K] are here
  for (int t = tid; t < n_bins; t += 256)
    if (hist[t]) atomicAdd(tables + t, (unsigned long long)hist[t]);
}

// agree of the maps [m0, m0 + cm) over the written consensus plane.  LDS: 1 + cm tiles, cm x 64 renumbering bytes, the
// bins [cm K K]
__global__ __launch_bounds__(256) void consensus_agree_kernel(ConsensusMaps maps, int m0, int cm, int identity, int K, int64_t n,
                                                              const uint8_t* __restrict__ cons,
                                                              unsigned long long* __restrict__ agree_out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint8_t* tiles = lds;                                // tile 0: the consensus
  uint8_t* ren = lds + (1 + cm) * CONS_PER_TRIP;
  unsigned* agree = reinterpret_cast<unsigned*>(ren + cm * 64);
  const int n_agree = cm * K * K, tid = threadIdx.x;
  for (int t = tid; t < n_agree; t += 256) agree[t] = 0;
  for (int t = tid; t < cm * 64; t += 256) ren[t] = maps.ren[m0 + (t >> 6)][t & 63];
  const unsigned one[4] = {1u, 1u, 1u, 1u};
  for (int64_t s = (int64_t)blockIdx.x * CONS_PER_TRIP; s < n; s += (int64_t)gridDim.x * CONS_PER_TRIP) {
    const int cnt = n - s < CONS_PER_TRIP ? (int)(n - s) : CONS_PER_TRIP;
    __syncthreads();
    stage_map(tiles, cons + s, cnt, nullptr, CONS_VOID);
    for (int m = 0; m < cm; ++m)
      stage_map(tiles + (1 + m) * CONS_PER_TRIP, maps.p[m0 + m] + s, cnt, identity ? nullptr : ren + m * 64, CONS_VOID);
    __syncthreads();
    const uint32_t wc = reinterpret_cast<const uint32_t*>(tiles)[tid];
    for (int m = 0; m < cm; ++m) {
      const uint32_t w = reinterpret_cast<const uint32_t*>(tiles + (1 + m) * CONS_PER_TRIP)[tid];
      int key[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = (wc >> (8 * e)) & 0xff;
        key[e] = c < K ? (m * K + c) * K + (int)((w >> (8 * e)) & 63) : -1;
      }
      wave_quad_add(agree, key, one);
    }
  }
  __syncthreads();
  for (int t = tid; t < n_agree; t += 256)
    if (agree[t]) atomicAdd(agree_out + (int64_t)m0 * K * K + t, (unsigned long long)agree[t]);
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_label_consensus(const uint8_t* const* labels_host, int M, const uint8_t* renumber_host_or_null, int K, int H, int W,
                          int diagonal, int64_t dist0, int min_support, uint8_t* consensus_dev, uint8_t* support_dev_or_null,
                          uint8_t* core_dev_or_null, int64_t* support_hist_host, int64_t* agree_host, int64_t* pair_host,
                          int64_t* bands_host, void* hip_stream) {
  PHMRF_CHECK(labels_host && consensus_dev && support_hist_host && agree_host && pair_host && bands_host, PHMRF_ERR_INVALID,
              "NULL buffer");
  PHMRF_CHECK(M >= 1, PHMRF_ERR_INVALID, "M must be >= 1");
  PHMRF_CHECK(M <= PHMRF_CONSENSUS_MAPS, PHMRF_ERR_UNSUPPORTED, "M must be <= 16");
  for (int m = 0; m < M; ++m) PHMRF_CHECK(labels_host[m], PHMRF_ERR_INVALID, "NULL map");
  PHMRF_TRY(check_states(K));
  PHMRF_CHECK(min_support >= 1 && min_support <= M, PHMRF_ERR_INVALID, "min_support must lie in [1, M]");
  PHMRF_CHECK(!(K == 64 && core_dev_or_null), PHMRF_ERR_INVALID, "K = 64 leaves no state number for the core plane's `unstable`");
  int64_t n;
  PHMRF_TRY(check_region(H, W, diagonal, &n));
  PHMRF_TRY(check_reach(dist0, H, W));
  PHMRF_TRY(check_nodes(n));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);

  ConsensusMaps maps = {};
  for (int m = 0; m < M; ++m) {
    maps.p[m] = labels_host[m];
    for (int l = 0; l < 64; ++l) {
      const int to = renumber_host_or_null ? renumber_host_or_null[m * 64 + l] : l;
      maps.ren[m][l] = (uint8_t)to;
      if (to < K) maps.allowed[m] |= 1ull << l;        // (255, "not a state of this map", is >= K)
    }
  }
  const int identity = renumber_host_or_null ? 0 : 1;
  const int KK = K * K;
  const int am = KK * M <= CONS_AGREE_BINS ? M : (CONS_AGREE_BINS / KK > 0 ? CONS_AGREE_BINS / KK : 1);
  const int n_hist = K * (M + 1), n_pair = M * M, n_bands = PHMRF_DIFF_BANDS * 3;
  const size_t n_tables = (size_t)n_hist + n_pair + n_bands + (size_t)M * KK;
  const int g = grid_of(n, CONS_PER_TRIP, CONS_GRID_CAP);

  Buffers buf;
  unsigned long long* tables;
  int* flag;
  PHMRF_TRY(buf.get(&tables, n_tables));
  PHMRF_TRY(buf.get(&flag, 1));
  PHMRF_HIP(hipMemsetAsync(tables, 0, n_tables * sizeof(unsigned long long), st));
  PHMRF_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  hipLaunchKernelGGL(consensus_check_kernel, dim3(g, M), dim3(256), 0, st, maps, n, flag);
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  PHMRF_CHECK(!(bad & 1), PHMRF_ERR_INVALID, "a label is >= 64");
  PHMRF_CHECK(!(bad & 2), PHMRF_ERR_INVALID, "a label is not a state of its map, or renumbers to a state >= K");

  const size_t lds_vote =
      (size_t)M * (CONS_PER_TRIP + 64) + sizeof(unsigned) * ((size_t)n_hist + n_pair + n_bands + (size_t)am * KK);
  hipLaunchKernelGGL(consensus_vote_kernel, dim3(g), dim3(256), lds_vote, st, maps, M, identity, K, n, W, diagonal,
                     (long long)dist0, min_support, am, consensus_dev, support_dev_or_null, core_dev_or_null, tables);
  PHMRF_HIP(hipGetLastError());
  unsigned long long* agree_dev = tables + n_hist + n_pair + n_bands;
  for (int m0 = am; m0 < M; m0 += am) {
    const int cm = M - m0 < am ? M - m0 : am;
    const size_t lds_agree = (size_t)(1 + cm) * CONS_PER_TRIP + (size_t)cm * 64 + sizeof(unsigned) * (size_t)cm * KK;
    hipLaunchKernelGGL(consensus_agree_kernel, dim3(g), dim3(256), lds_agree, st, maps, m0, cm, identity, K, n, consensus_dev,
                       agree_dev);
    PHMRF_HIP(hipGetLastError());
  }
  std::vector<unsigned long long> got(n_tables);
  PHMRF_HIP(hipMemcpyAsync(got.data(), tables, n_tables * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  const unsigned long long* p = got.data();
  for (int t = 0; t < n_hist; ++t) support_hist_host[t] = (int64_t)p[t];
  p += n_hist;
  for (int a = 0; a < M; ++a)
    for (int b = 0; b < M; ++b) pair_host[a * M + b] = a == b ? n : (int64_t)p[a < b ? a * M + b : b * M + a];
  p += n_pair;
  for (int t = 0; t < n_bands; ++t) bands_host[t] = (int64_t)p[t];
  p += n_bands;
  for (size_t t = 0; t < (size_t)M * KK; ++t) agree_host[t] = (int64_t)p[t];
  return PHMRF_OK;
}

}  // extern "C"
