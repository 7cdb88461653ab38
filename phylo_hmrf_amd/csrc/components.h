// What the calls that LIST grid components share (smooth.hip: the small ones, compare.hip: the differential domains,
// domains.hip: the domains of one map): the label check, the full-matrix area of every component, the compact ids of the
// listed roots, the most frequent state of a histogram row and the (min, max) bounds of the listed components.
//
//   area     acc[root] += (weight << 32) | 1 per counted node (weight 1 on the diagonal, 2 elsewhere), mirror[root] = 1 if a
//            node has j - i <= 1 (component_area, runs.h).  components_area_kernel: one packed atomic per run of equal root
//            among consecutive lanes.  domains.hip has a kernel of its own, with the same rule, for maps whose components
//            hold millions of nodes.
//   ids      every workgroup owns `chunk` consecutive nodes.  count_listed counts the listed roots among them, hand_out_ids
//            gives them consecutive ids in node order from an offset.  Where the order of the ids is part of the result the
//            workgroups' counts are written out (components_count_kernel, or a kernel of the caller's that counts more:
//            domains.hip), summed in workgroup order (components_scan_kernel) and the ids handed out from those offsets
//            (components_compact_kernel).  Where it is not, one kernel takes a workgroup's ids with ONE atomic between the
//            two steps (smooth.hip).
//
// The kernels are compiled into every file that launches them, like the kernels of that file's own.

#pragma once

#include "runs.h"

namespace phmrf {

// the node predicate of an area pass: every node ...
struct EveryNode {
  __device__ __forceinline__ bool operator()(int64_t) const { return true; }
};
// ... or the nodes where diff (compare.hip) is 2
struct DiffNode {
  const uint8_t* __restrict__ diff;
  __device__ __forceinline__ bool operator()(int64_t v) const { return diff[v] == 2; }
};

// Is root v listed: its area on the full matrix within [min_area, max_area] and, with a diff map, its value there 2
struct ListedRoot {
  const uint8_t* __restrict__ diff;                    // null: a root of any value
  int diagonal;
  const unsigned long long* __restrict__ acc;
  const uint8_t* __restrict__ mirror;
  long long min_area, max_area;
  __device__ __forceinline__ bool operator()(int64_t v) const {
    if (diff && diff[v] != 2) return false;
    const long long area = component_area(v, diagonal, acc, mirror);
    return area >= min_area && area <= max_area;
  }
};
constexpr long long ANY_AREA = 0x7fffffffffffffffll;   // a max_area that excludes nothing

// the nodes [*start, *end) of this workgroup
__device__ __forceinline__ void group_chunk(int64_t n, int64_t chunk, int64_t* start, int64_t* end) {
  *start = (int64_t)blockIdx.x * chunk;
  *end = *start + chunk < n ? *start + chunk : n;
}

// -> the listed roots among the nodes [start, end), the same number in every lane of the workgroup (256 lanes, all of which
// call it); per_root(v) runs for every root, listed or not.  wave_cnt: LDS [4]
template <typename PerRoot>
__device__ __forceinline__ int count_listed(const int32_t* __restrict__ comp, int64_t start, int64_t end, const ListedRoot& listed,
                                            int* wave_cnt, PerRoot per_root) {
  int mine = 0;
  for (int64_t v = start + threadIdx.x; v < end; v += 256)
    if (comp[v] == (int)v) {
      mine += listed(v);
      per_root(v);
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = mine;
  __syncthreads();
  return wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// cid[root] = base, base + 1, ... for the listed roots of [start, end) in node order, -1 for any other root (roots only:
// nothing reads cid elsewhere); roots[id] = root for id < cap (roots null: no list).  wave_cnt: LDS [4], read by every lane
// before the call's first barrier
__device__ __forceinline__ void hand_out_ids(const int32_t* __restrict__ comp, int64_t start, int64_t end, const ListedRoot& listed,
                                             int base, int* wave_cnt, int32_t* __restrict__ cid, int32_t* __restrict__ roots,
                                             int64_t cap) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int64_t b0 = start; b0 < end; b0 += 256) {
    const int64_t v = b0 + threadIdx.x;
    const bool root = v < end && comp[v] == (int)v;
    const bool take = root && listed(v);
    const unsigned long long mask = __ballot(take);
    __syncthreads();                                   // (wave_cnt of the previous trip has been read)
    if (lane == 0) wave_cnt[wid] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wid; ++w) off += wave_cnt[w];
    if (root) {
      const int id = take ? off + __popcll(mask & (lanes_at_or_below(lane) >> 1)) : -1;
      cid[v] = id;
      if (roots && id >= 0 && id < cap) roots[id] = (int32_t)v;
    }
    base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
  }
}

// the most frequent state of a K-bin histogram row (strictly greater wins: the lowest state wins a tie; 0 for an empty
// row), its count and the row's sum
struct Mode {
  int state;
  unsigned long long best, total;
};
__device__ __forceinline__ Mode mode_of(const unsigned long long* __restrict__ row, int K) {
  Mode m = {0, 0, 0};
  for (int q = 0; q < K; ++q) {
    const unsigned long long c = row[q];
    m.total += c;
    if (c > m.best) {
      m.best = c;
      m.state = q;
    }
  }
  return m;
}

// e[0] = min(e[0], lo), e[1] = max(e[1], hi)  (a stale read only costs an atomic: the bounds move one way)
__device__ __forceinline__ void widen(int* __restrict__ e, int lo, int hi) {
  if (lo < e[0]) atomicMin(e, lo);
  if (hi > e[1]) atomicMax(e + 1, hi);
}

namespace {

// bad |= 1 for a label >= K, 2 for a confidence that is not a finite number in [0, 1] (conf null: none given)
__global__ __launch_bounds__(256) void components_check_kernel(const uint8_t* __restrict__ labels, const float* __restrict__ conf,
                                                               int64_t n, int K, int* __restrict__ bad) {
  int wrong = 0;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
    if ((int)labels[v] >= K) wrong |= 1;
    if (conf && !unit_conf(conf[v])) wrong |= 2;
  }
  if (wrong) atomicOr(bad, wrong);
}

// The areas of the components over the counted nodes.  Where few nodes count (two maps mostly agree, so the diff map's
// component of value 0 holds nearly every node: counted too, every wave's atomic would land on its one root, 61 % of a
// compare call's kernel time, measured) the waves without one skip the add; with every node counted that drops the trips past n.
template <typename Counted>
__global__ __launch_bounds__(256) void components_area_kernel(const int32_t* __restrict__ comp, Counted counted, int64_t n, int W,
                                                              int diagonal, unsigned long long* __restrict__ acc,
                                                              uint8_t* __restrict__ mirror) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) - lane; base < n; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = base + lane;
    int key = -1;
    unsigned long long x = 0;
    if (v < n && counted(v)) {
      int i, j;
      grid_coords(v, W, diagonal, &i, &j);
      key = comp[v];
      x = ((unsigned long long)(diagonal && i == j ? 1 : 2) << 32) | 1ull;
      if (diagonal && j - i <= 1 && !mirror[key]) mirror[key] = 1;
    }
    if (__ballot(key >= 0) == 0ull) continue;           // (the same for the whole wave)
    wave_run_add(acc, key, x);                          // one packed atomic per run of equal root among consecutive lanes
  }
}

// per_group[g] = listed roots among workgroup g's nodes
__global__ __launch_bounds__(256) void components_count_kernel(const int32_t* __restrict__ comp, int64_t n, int64_t chunk,
                                                               ListedRoot listed, int* __restrict__ per_group) {
  __shared__ int wave_cnt[4];
  int64_t start, end;
  group_chunk(n, chunk, &start, &end);
  const int total = count_listed(comp, start, end, listed, wave_cnt, [](int64_t) {});
  if (threadIdx.x == 0) per_group[blockIdx.x] = total;
}

// exclusive prefix sum of per_group[0 .. g) in place (g <= 4096: one workgroup), *count = the total
__global__ __launch_bounds__(256) void components_scan_kernel(int* __restrict__ per_group, int g, int* __restrict__ count) {
  __shared__ int part[256];
  const int per = (g + 255) / 256, lo = threadIdx.x * per, hi = lo + per < g ? lo + per : g;
  int s = 0;
  for (int t = lo; t < hi; ++t) s += per_group[t];
  part[threadIdx.x] = s;
  __syncthreads();
  int before = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) before += part[t];
  for (int t = lo; t < hi; ++t) {
    const int c = per_group[t];
    per_group[t] = before;
    before += c;
  }
  if (threadIdx.x == 255) *count = before;
}

// the ids of the listed roots in ascending order of the roots, from the scanned per_group
__global__ __launch_bounds__(256) void components_compact_kernel(const int32_t* __restrict__ comp, int64_t n, int64_t chunk,
                                                                 ListedRoot listed, const int* __restrict__ per_group, int64_t cap,
                                                                 int32_t* __restrict__ cid, int32_t* __restrict__ roots) {
  __shared__ int wave_cnt[4];
  int64_t start, end;
  group_chunk(n, chunk, &start, &end);
  hand_out_ids(comp, start, end, listed, per_group[blockIdx.x], wave_cnt, cid, roots, cap);
}

// bounds[2p], bounds[2p + 1] = an empty (min, max) pair
__global__ __launch_bounds__(256) void components_bounds_init_kernel(int* __restrict__ bounds, int64_t pairs) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += (int64_t)gridDim.x * blockDim.x) {
    bounds[2 * p] = 0x7fffffff;
    bounds[2 * p + 1] = -1;
  }
}

}  // namespace
}  // namespace phmrf
