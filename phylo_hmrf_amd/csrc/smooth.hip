// gfx950 kernels of the post-processing's small-region smoothing (phmrf_smooth_labels; the reference's
// processing/small_region_test.m with query_neighbor_state_test.m).
//
// One pass (Jacobi: every decision reads the map as it was at the start of the pass) on one region's u8 labels:
//
//   components   8-connected components of equal label on the grid (moves.hip's union-find, launch_grid_components):
//                comp[v] = the smallest node id of v's component
//   area         per root: the component's area on the FULL matrix.  A diagonal block stores the upper triangle; two of its
//                nodes are 8-adjacent on the full matrix (directly or through a mirror) exactly when they are 8-adjacent in
//                the upper triangle, so a component is either its own mirror -- exactly when it holds a node with
//                j - i <= 1 -- with area 2 * (nodes) - (diagonal nodes), or it has a separate mirror twin of the same area
//                that reaches the same decision.  One packed 64-bit atomic per run of equal root in a wave.
//   compact      roots with area <= max_area get consecutive ids (one atomic per workgroup); the vote histograms are sized by
//                their number
//   vote         every node of a small component whose (2h+1) x (2h+1) window lies inside the matrix adds, with weight 2 for
//                an off-diagonal node of a self-mirror component (its mirror pixel's window is the transpose of its own) and
//                1 otherwise, every window state != its own to the component's K-bin histogram.  A window pixel (x, y) of a
//                diagonal block reads node (min(x, y), max(x, y)).  Runs of equal state in the window go in as one atomic.
//   decide       per small component: the most frequent state k (the lowest on ties) when 2 count(k) > collected
//   apply        out[v] = k for every node of a relabelled component
//
// All counts are integers: the result does not depend on the order in which the atomics land.

#include "runs.h"

namespace phmrf {
namespace {

// *bad = 1 if any label >= K
__global__ __launch_bounds__(256) void smooth_check_kernel(const uint8_t* __restrict__ labels, int64_t n, int K,
                                                           int* __restrict__ bad) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x)
    if ((int)labels[v] >= K) {
      atomicOr(bad, 1);
      return;
    }
}

// acc[root] += (weight << 32) | 1 per node (weight 1 on the diagonal, 2 elsewhere), mirror[root] = 1 if j - i <= 1
__global__ __launch_bounds__(256) void smooth_area_kernel(const int32_t* __restrict__ comp, int64_t n, int W, int diagonal,
                                                          unsigned long long* __restrict__ acc, uint8_t* __restrict__ mirror) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) - lane; base < n; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = base + lane;
    int key = -1;
    unsigned long long x = 0;
    if (v < n) {
      int i, j;
      grid_coords(v, W, diagonal, &i, &j);
      key = comp[v];
      x = ((unsigned long long)(diagonal && i == j ? 1 : 2) << 32) | 1ull;
      if (diagonal && j - i <= 1) mirror[key] = 1;
    }
    wave_run_add(acc, key, x);                 // one packed atomic per run of equal root among consecutive lanes
  }
}

__device__ __forceinline__ bool small_root(const int32_t* __restrict__ comp, int64_t v, int diagonal,
                                           const unsigned long long* __restrict__ acc, const uint8_t* __restrict__ mirror,
                                           long long max_area) {
  return component_area(v, diagonal, acc, mirror) <= max_area;
}

// cid[root] = compact id of a small component, -1 for a large one (roots only: nothing reads cid elsewhere).  Every
// workgroup owns `chunk` consecutive nodes: it counts its small roots, takes their ids with ONE atomic, then hands them out
// in node order (an atomic per wave on the one counter would serialise: 1.4 M of them at 88.8 M nodes)
__global__ __launch_bounds__(256) void smooth_compact_kernel(const int32_t* __restrict__ comp, int64_t n, int64_t chunk,
                                                             int diagonal, const unsigned long long* __restrict__ acc,
                                                             const uint8_t* __restrict__ mirror, long long max_area,
                                                             int32_t* __restrict__ cid, int* __restrict__ count) {
  __shared__ int wave_cnt[4];
  __shared__ int base_s;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t start = (int64_t)blockIdx.x * chunk, end = start + chunk < n ? start + chunk : n;
  int mine = 0;
  for (int64_t v = start + threadIdx.x; v < end; v += 256)
    mine += comp[v] == (int)v && small_root(comp, v, diagonal, acc, mirror, max_area);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
  if (lane == 0) wave_cnt[wid] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    base_s = total ? atomicAdd(count, total) : 0;
  }
  __syncthreads();
  int base = base_s;
  for (int64_t b0 = start; b0 < end; b0 += 256) {
    const int64_t v = b0 + threadIdx.x;
    const bool root = v < end && comp[v] == (int)v;
    const bool small = root && small_root(comp, v, diagonal, acc, mirror, max_area);
    const unsigned long long mask = __ballot(small);
    __syncthreads();                                   // (wave_cnt of the previous trip has been read)
    if (lane == 0) wave_cnt[wid] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wid; ++w) off += wave_cnt[w];
    if (root) cid[v] = small ? off + __popcll(mask & (lanes_at_or_below(lane) >> 1)) : -1;
    base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
  }
}

__device__ __forceinline__ int label_at(const uint8_t* __restrict__ labels, int x, int y, int W, int diagonal) {
  if (!diagonal) return labels[(int64_t)x * W + y];
  const int a = x < y ? x : y, b = x < y ? y : x;
  return labels[grid_row_base(a, W, 1) + b];
}

__global__ __launch_bounds__(256) void smooth_vote_kernel(const uint8_t* __restrict__ labels, const int32_t* __restrict__ comp,
                                                          const int32_t* __restrict__ cid, const uint8_t* __restrict__ mirror,
                                                          int64_t n, int H, int W, int diagonal, int K, int h,
                                                          unsigned long long* __restrict__ hist) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
    const int r = comp[v];
    const int c = cid[r];
    if (c < 0) continue;
    int i, j;
    grid_coords(v, W, diagonal, &i, &j);
    if (i < h || i > H - 1 - h || j < h || j > W - 1 - h) continue;     // the window crosses the border: no vote
    const unsigned long long wt = (diagonal && i != j && mirror[r]) ? 2ull : 1ull;
    const int s = labels[v];
    unsigned long long* row = hist + (int64_t)c * K;
    int cur = -1;
    unsigned long long run = 0;
    for (int x = i - h; x <= i + h; ++x)
      for (int y = j - h; y <= j + h; ++y) {
        const int q = label_at(labels, x, y, W, diagonal);
        if (q == s) continue;
        if (q == cur) {
          ++run;
        } else {
          if (run) atomicAdd(row + cur, run * wt);
          cur = q;
          run = 1;
        }
      }
    if (run) atomicAdd(row + cur, run * wt);
  }
}

// dec[c] = the new state of small component c, 0xff = keeps its own; counters[0] += relabelled components
__global__ __launch_bounds__(256) void smooth_decide_kernel(const unsigned long long* __restrict__ hist, int count, int K,
                                                            uint8_t* __restrict__ dec, unsigned long long* __restrict__ counters) {
  unsigned long long relabelled = 0;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < count; c += gridDim.x * blockDim.x) {
    const unsigned long long* row = hist + (int64_t)c * K;
    unsigned long long total = 0, best = 0;
    int k = 0;
    for (int q = 0; q < K; ++q) {
      const unsigned long long m = row[q];
      total += m;
      if (m > best) {               // strictly: the lowest state wins a tie
        best = m;
        k = q;
      }
    }
    const bool change = total > 0 && 2ull * best > total;
    dec[c] = change ? (uint8_t)k : (uint8_t)0xff;
    relabelled += change;
  }
  wave_add(counters, relabelled);
}

// counters[1] += nodes changed
__global__ __launch_bounds__(256) void smooth_apply_kernel(const int32_t* __restrict__ comp, const int32_t* __restrict__ cid,
                                                           const uint8_t* __restrict__ dec, int64_t n, uint8_t* __restrict__ out,
                                                           unsigned long long* __restrict__ counters) {
  unsigned long long changed = 0;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
    const int c = cid[comp[v]];
    if (c >= 0 && dec[c] != 0xff) {
      out[v] = dec[c];
      ++changed;
    }
  }
  wave_add(counters + 1, changed);
}

// device buffers of one call, released on every way out
struct SmoothWork {
  int32_t* comp = nullptr;
  int32_t* cid = nullptr;
  unsigned long long* acc = nullptr;
  uint8_t* mirror = nullptr;
  uint8_t* cur = nullptr;
  unsigned long long* hist = nullptr;
  uint8_t* dec = nullptr;
  unsigned long long* counters = nullptr;
  int* scalars = nullptr;          // [0] bad label, [1] number of small components
  int64_t hist_cap = 0;            // components the histograms hold
  ~SmoothWork() {
    void* all[] = {comp, cid, acc, mirror, cur, hist, dec, counters, scalars};
    for (void* p : all)
      if (p) (void)hipFree(p);
  }
};

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_smooth_labels(const uint8_t* labels_dev, uint8_t* out_dev, int H, int W, int diagonal, int K, int window,
                        int64_t max_area, int n_iter, int64_t* counts_host, void* hip_stream) {
  PHMRF_CHECK(labels_dev && out_dev, PHMRF_ERR_INVALID, "NULL label buffer");
  PHMRF_CHECK(H >= 1 && W >= 1, PHMRF_ERR_INVALID, "H and W must be >= 1");
  PHMRF_CHECK(diagonal == 0 || diagonal == 1, PHMRF_ERR_INVALID, "diagonal must be 0 or 1");
  PHMRF_CHECK(!diagonal || H == W, PHMRF_ERR_INVALID, "a diagonal block is square (H == W)");
  PHMRF_CHECK(K >= 1, PHMRF_ERR_INVALID, "K must be >= 1");
  PHMRF_CHECK(K <= 64, PHMRF_ERR_UNSUPPORTED, "K must be <= 64");
  PHMRF_CHECK(window >= 1, PHMRF_ERR_INVALID, "window must be >= 1");
  PHMRF_CHECK(n_iter >= 0, PHMRF_ERR_INVALID, "n_iter must be >= 0");
  const int64_t n = diagonal ? (int64_t)W * (W + 1) / 2 : (int64_t)H * W;
  PHMRF_CHECK(n < ((int64_t)1 << 31) - 64, PHMRF_ERR_UNSUPPORTED, "the region must have fewer than 2^31 - 64 nodes");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int h = window / 2;
  const int g = grid_of(n);
  const int64_t chunk = ((n + g - 1) / g + 255) / 256 * 256;     // smooth_compact_kernel: consecutive nodes per workgroup

  SmoothWork w;
  PHMRF_TRY(alloc(&w.scalars, 2));
  PHMRF_HIP(hipMemsetAsync(w.scalars, 0, 2 * sizeof(int), st));
  hipLaunchKernelGGL(smooth_check_kernel, dim3(g), dim3(256), 0, st, labels_dev, n, K, w.scalars);
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_HIP(hipMemcpyAsync(&bad, w.scalars, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  PHMRF_CHECK(!bad, PHMRF_ERR_INVALID, "a label is >= K");

  if (labels_dev != out_dev) PHMRF_HIP(hipMemcpyAsync(out_dev, labels_dev, (size_t)n, hipMemcpyDeviceToDevice, st));
  if (n_iter == 0) {
    PHMRF_HIP(hipStreamSynchronize(st));
    return PHMRF_OK;
  }
  PHMRF_TRY(alloc(&w.comp, (size_t)n));
  PHMRF_TRY(alloc(&w.cid, (size_t)n));
  PHMRF_TRY(alloc(&w.acc, (size_t)n));
  PHMRF_TRY(alloc(&w.mirror, (size_t)n));
  PHMRF_TRY(alloc(&w.cur, (size_t)n));
  PHMRF_TRY(alloc(&w.counters, (size_t)2 * n_iter));
  PHMRF_HIP(hipMemsetAsync(w.counters, 0, (size_t)2 * n_iter * sizeof(unsigned long long), st));
  std::vector<int64_t> small(n_iter, 0);

  for (int it = 0; it < n_iter; ++it) {
    // the pass reads the map as it was at its start (cur) and writes its changes into out
    PHMRF_HIP(hipMemcpyAsync(w.cur, out_dev, (size_t)n, hipMemcpyDeviceToDevice, st));
    PHMRF_TRY(launch_grid_components(w.comp, n, W, diagonal, w.cur, st));
    PHMRF_HIP(hipMemsetAsync(w.acc, 0, (size_t)n * sizeof(unsigned long long), st));
    PHMRF_HIP(hipMemsetAsync(w.mirror, 0, (size_t)n, st));
    PHMRF_HIP(hipMemsetAsync(w.scalars + 1, 0, sizeof(int), st));
    hipLaunchKernelGGL(smooth_area_kernel, dim3(g), dim3(256), 0, st, w.comp, n, W, diagonal, w.acc, w.mirror);
    hipLaunchKernelGGL(smooth_compact_kernel, dim3(g), dim3(256), 0, st, w.comp, n, chunk, diagonal, w.acc, w.mirror,
                       (long long)max_area, w.cid, w.scalars + 1);
    PHMRF_HIP(hipGetLastError());
    int count = 0;
    PHMRF_HIP(hipMemcpyAsync(&count, w.scalars + 1, sizeof(int), hipMemcpyDeviceToHost, st));
    PHMRF_HIP(hipStreamSynchronize(st));
    small[it] = count;
    if (count == 0) continue;
    if (count > w.hist_cap) {
      if (w.hist) PHMRF_HIP(hipFree(w.hist));
      if (w.dec) PHMRF_HIP(hipFree(w.dec));
      w.hist = nullptr;
      w.dec = nullptr;
      PHMRF_TRY(alloc(&w.hist, (size_t)count * K));
      PHMRF_TRY(alloc(&w.dec, (size_t)count));
      w.hist_cap = count;
    }
    PHMRF_HIP(hipMemsetAsync(w.hist, 0, (size_t)count * K * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(smooth_vote_kernel, dim3(g), dim3(256), 0, st, w.cur, w.comp, w.cid, w.mirror, n, H, W, diagonal, K, h,
                       w.hist);
    hipLaunchKernelGGL(smooth_decide_kernel, dim3(grid_of(count)), dim3(256), 0, st, w.hist, count, K, w.dec,
                       w.counters + 2 * it);
    hipLaunchKernelGGL(smooth_apply_kernel, dim3(g), dim3(256), 0, st, w.comp, w.cid, w.dec, n, out_dev, w.counters + 2 * it);
    PHMRF_HIP(hipGetLastError());
  }
  std::vector<unsigned long long> cnt((size_t)2 * n_iter);
  PHMRF_HIP(hipMemcpyAsync(cnt.data(), w.counters, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  if (counts_host)
    for (int it = 0; it < n_iter; ++it) {
      counts_host[3 * it] = small[it];
      counts_host[3 * it + 1] = (int64_t)cnt[2 * it];
      counts_host[3 * it + 2] = (int64_t)cnt[2 * it + 1];
    }
  return PHMRF_OK;
}

}  // extern "C"
