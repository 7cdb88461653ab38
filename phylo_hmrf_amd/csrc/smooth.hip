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
//                that reaches the same decision.  One packed 64-bit atomic per run of equal root in a wave
//                (components_area_kernel over every node, components.h).
//   compact      roots with area <= max_area get consecutive ids (count_listed and hand_out_ids of components.h in one
//                kernel, one atomic per workgroup between them); the vote histograms are sized by their number
//   vote         every node of a small component whose (2h+1) x (2h+1) window lies inside the matrix adds, with weight 2 for
//                an off-diagonal node of a self-mirror component (its mirror pixel's window is the transpose of its own) and
//                1 otherwise, every window state != its own to the component's K-bin histogram.  A window pixel (x, y) of a
//                diagonal block reads node (min(x, y), max(x, y)).  Runs of equal state in the window go in as one atomic.
//   decide       per small component: the most frequent state k (the lowest on ties) when 2 count(k) > collected
//   apply        out[v] = k for every node of a relabelled component
//
// All counts are integers: the result does not depend on the order in which the atomics land.

#include "components.h"

namespace phmrf {
namespace {

// cid[root] = compact id of a small component, -1 for a large one.  Every workgroup owns `chunk` consecutive nodes: it
// counts its small roots, takes their ids with ONE atomic, then hands them out in node order (an atomic per wave on the one
// counter would serialise: 1.4 M of them at 88.8 M nodes)
__global__ __launch_bounds__(256) void smooth_compact_kernel(const int32_t* __restrict__ comp, int64_t n, int64_t chunk,
                                                             ListedRoot small, int32_t* __restrict__ cid, int* __restrict__ count) {
  __shared__ int wave_cnt[4];
  __shared__ int base_s;
  int64_t start, end;
  group_chunk(n, chunk, &start, &end);
  const int total = count_listed(comp, start, end, small, wave_cnt, [](int64_t) {});
  if (threadIdx.x == 0) base_s = total ? atomicAdd(count, total) : 0;
  __syncthreads();
  hand_out_ids(comp, start, end, small, base_s, wave_cnt, cid, nullptr, 0);
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
    const Mode m = mode_of(hist + (int64_t)c * K, K);
    const bool change = m.total > 0 && 2ull * m.best > m.total;
    dec[c] = change ? (uint8_t)m.state : (uint8_t)0xff;
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

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_smooth_labels(const uint8_t* labels_dev, uint8_t* out_dev, int H, int W, int diagonal, int K, int window,
                        int64_t max_area, int n_iter, int64_t* counts_host, void* hip_stream) {
  PHMRF_CHECK(labels_dev && out_dev, PHMRF_ERR_INVALID, "NULL label buffer");
  int64_t n;
  PHMRF_TRY(check_region(H, W, diagonal, &n));
  PHMRF_TRY(check_states(K));
  PHMRF_CHECK(window >= 1, PHMRF_ERR_INVALID, "window must be >= 1");
  PHMRF_CHECK(n_iter >= 0, PHMRF_ERR_INVALID, "n_iter must be >= 0");
  PHMRF_TRY(check_nodes(n));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int h = window / 2;
  const int g = grid_of(n);
  const int64_t chunk = ((n + g - 1) / g + 255) / 256 * 256;     // smooth_compact_kernel: consecutive nodes per workgroup

  Buffers buf;
  int* scalars;                    // [0] bad label, [1] number of small components
  PHMRF_TRY(buf.get(&scalars, 2));
  PHMRF_HIP(hipMemsetAsync(scalars, 0, 2 * sizeof(int), st));
  hipLaunchKernelGGL(components_check_kernel, dim3(g), dim3(256), 0, st, labels_dev, (const float*)nullptr, n, K, scalars);
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_HIP(hipMemcpyAsync(&bad, scalars, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  PHMRF_CHECK(!bad, PHMRF_ERR_INVALID, "a label is >= K");

  if (labels_dev != out_dev) PHMRF_HIP(hipMemcpyAsync(out_dev, labels_dev, (size_t)n, hipMemcpyDeviceToDevice, st));
  if (n_iter == 0) {
    PHMRF_HIP(hipStreamSynchronize(st));
    return PHMRF_OK;
  }
  int32_t *comp, *cid;
  unsigned long long *acc, *counters, *hist = nullptr;
  uint8_t *mirror, *cur, *dec = nullptr;
  int64_t hist_cap = 0;            // components the histograms hold
  PHMRF_TRY(buf.get(&comp, (size_t)n));
  PHMRF_TRY(buf.get(&cid, (size_t)n));
  PHMRF_TRY(buf.get(&acc, (size_t)n));
  PHMRF_TRY(buf.get(&mirror, (size_t)n));
  PHMRF_TRY(buf.get(&cur, (size_t)n));
  PHMRF_TRY(buf.get(&counters, (size_t)2 * n_iter));
  PHMRF_HIP(hipMemsetAsync(counters, 0, (size_t)2 * n_iter * sizeof(unsigned long long), st));
  std::vector<int64_t> small(n_iter, 0);
  const ListedRoot is_small = {nullptr, diagonal, acc, mirror, 0, (long long)max_area};

  for (int it = 0; it < n_iter; ++it) {
    // the pass reads the map as it was at its start (cur) and writes its changes into out
    PHMRF_HIP(hipMemcpyAsync(cur, out_dev, (size_t)n, hipMemcpyDeviceToDevice, st));
    PHMRF_TRY(launch_grid_components(comp, n, W, diagonal, cur, st));
    PHMRF_HIP(hipMemsetAsync(acc, 0, (size_t)n * sizeof(unsigned long long), st));
    PHMRF_HIP(hipMemsetAsync(mirror, 0, (size_t)n, st));
    PHMRF_HIP(hipMemsetAsync(scalars + 1, 0, sizeof(int), st));
    hipLaunchKernelGGL(components_area_kernel<EveryNode>, dim3(g), dim3(256), 0, st, comp, EveryNode(), n, W, diagonal, acc, mirror);
    hipLaunchKernelGGL(smooth_compact_kernel, dim3(g), dim3(256), 0, st, comp, n, chunk, is_small, cid, scalars + 1);
    PHMRF_HIP(hipGetLastError());
    int count = 0;
    PHMRF_HIP(hipMemcpyAsync(&count, scalars + 1, sizeof(int), hipMemcpyDeviceToHost, st));
    PHMRF_HIP(hipStreamSynchronize(st));
    small[it] = count;
    if (count == 0) continue;
    if (count > hist_cap) {
      PHMRF_TRY(buf.release(&hist));
      PHMRF_TRY(buf.release(&dec));
      PHMRF_TRY(buf.get(&hist, (size_t)count * K));
      PHMRF_TRY(buf.get(&dec, (size_t)count));
      hist_cap = count;
    }
    PHMRF_HIP(hipMemsetAsync(hist, 0, (size_t)count * K * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(smooth_vote_kernel, dim3(g), dim3(256), 0, st, cur, comp, cid, mirror, n, H, W, diagonal, K, h, hist);
    hipLaunchKernelGGL(smooth_decide_kernel, dim3(grid_of(count)), dim3(256), 0, st, hist, count, K, dec, counters + 2 * it);
    hipLaunchKernelGGL(smooth_apply_kernel, dim3(g), dim3(256), 0, st, comp, cid, dec, n, out_dev, counters + 2 * it);
    PHMRF_HIP(hipGetLastError());
  }
  std::vector<unsigned long long> cnt((size_t)2 * n_iter);
  PHMRF_HIP(hipMemcpyAsync(cnt.data(), counters, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
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
