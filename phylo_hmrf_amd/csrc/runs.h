// What the post-processing's kernel files share (smooth.hip, compare.hip, profile.hip, domains.hip, tracks.hip, enrich.hip):
// the capped grid, the wave helpers of their integer accumulations -- one atomic per RUN of equal destination among
// consecutive lanes, because state maps are piecewise constant --, the split of a label row into aligned words (tracks.hip,
// enrich.hip) and the full-matrix area of a grid component.
#pragma once

#include "common.h"

namespace phmrf {

inline int grid_of(int64_t n, int tb = 256, int cap = 256 * 16) {
  int64_t g = (n + tb - 1) / tb;
  if (g > cap) g = cap;
  return g < 1 ? 1 : (int)g;
}

__device__ __forceinline__ unsigned long long lanes_at_or_below(int lane) {
  return lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
}

__device__ __forceinline__ void wave_add(unsigned long long* dst, unsigned long long x) {   // one atomic per wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, x);
}

// dst[key] += x, one atomic per run of equal key among consecutive lanes (key < 0: the lane adds nothing).  Every lane of
// the wave must call it.  Inclusive prefix sum, each run's last lane adds the run's part.
template <typename T>
__device__ __forceinline__ void wave_run_add(T* dst, int key, T x) {
  const int lane = threadIdx.x & 63;
  const int key_prev = __shfl_up(key, 1, 64);
  const bool head = lane == 0 || key_prev != key;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T t = __shfl_up(x, off, 64);
    if (lane >= off) x += t;
  }
  const unsigned long long heads = __ballot(head);
  const int h = 63 - __clzll((long long)(heads & lanes_at_or_below(lane)));
  const T before = __shfl(x, h > 0 ? h - 1 : 0, 64);
  const bool next_head = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  if (key >= 0 && next_head) atomicAdd(dst + key, x - (h > 0 ? before : (T)0));
}

// The stored cells of storage row i of a label map between the columns j0 and j1 (a diagonal block: from the diagonal on):
// columns [ja, ja + nc) at p; `head` bytes (at most three) up to the next 4-byte boundary of the address, nvec aligned words of
// four labels, then the bytes from `tail` on: nbytes = head + what follows the words.  A region's slice of a state_vec starts at
// any byte and a diagonal block's rows shift by one node each, so every row has its own head.
struct LabelRow {
  const uint8_t* p;
  int ja, head, nvec, tail, nbytes;
};

__device__ __forceinline__ LabelRow label_row(const uint8_t* __restrict__ labels, int i, int j0, int j1, int W, int diagonal) {
  LabelRow r;
  r.ja = (diagonal && j0 < i) ? i : j0;
  const int nc = j1 - r.ja;                            // >= 1 is the caller's business
  r.p = labels + grid_id<int64_t>(i, r.ja, W, diagonal);
  r.head = (int)((4 - (reinterpret_cast<uintptr_t>(r.p) & 3)) & 3);
  if (r.head > nc) r.head = nc;
  r.nvec = (nc - r.head) >> 2;
  r.tail = r.head + 4 * r.nvec;
  r.nbytes = r.head + (nc - r.tail);
  return r;
}

// band of a distance d >= 0: 0 for d == 0, else t with 2^(t-1) <= d < 2^t (PHMRF_DIFF_BANDS of them below 2^31)
__device__ __forceinline__ int band_of(long long d) { return d == 0 ? 0 : 64 - __clzll(d); }

// the area on the full matrix of the component with root v, from acc[v] = (weight << 32) | nodes (weight: 1 per diagonal
// node, 2 per other node) and mirror[v] = a node has j - i <= 1: a diagonal block's component that is its own mirror counts
// its off-diagonal nodes twice, any other component its stored nodes
__device__ __forceinline__ long long component_area(int64_t v, int diagonal, const unsigned long long* __restrict__ acc,
                                                    const uint8_t* __restrict__ mirror) {
  const unsigned long long a = acc[v];
  return (diagonal && mirror[v]) ? (long long)(a >> 32) : (long long)(a & 0xffffffffull);
}

// a finite float32 in [0, 1], told by its bits (the library is compiled with -fno-honor-nans: a comparison proves nothing
// about a NaN): +0 .. 1.0 are the patterns up to 0x3f800000, and -0
__host__ __device__ __forceinline__ bool unit_bits(uint32_t u) { return u <= 0x3f800000u || u == 0x80000000u; }
__device__ __forceinline__ bool unit_conf(float c) { return unit_bits(__float_as_uint(c)); }

template <typename T>
int alloc(T** p, size_t count) {
  PHMRF_HIP(hipMalloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T)));
  return PHMRF_OK;
}

}  // namespace phmrf
