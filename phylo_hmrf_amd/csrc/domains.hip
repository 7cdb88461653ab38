// gfx950 kernels that describe ONE state map of one region (phmrf_state_adjacency, phmrf_state_domains; DESIGN.md
// section 7).  Integer arithmetic throughout: no result depends on the order in which the atomics land.
//
//   adjacency    per stored edge of the 8-neighbour grid graph, counts[a, b] with a the state of the edge's first node:
//                every node looks at its four forward neighbours; each workgroup keeps a K x K table of u32 bins in LDS (at
//                most 16 KB), ONE LDS atomic per run of equal (a, b) among consecutive lanes (wave_run_add), and flushes
//                its non-zero bins with u64 global atomics.  The call folds the table into the symmetric one on the host.
//   check        a label >= K, a confidence that is not a finite number in [0, 1] (components_check_kernel)
//   components   moves.hip's union-find on the map itself (launch_grid_components)
//   areas        components_area_kernel's rule, every node counted.  A state map always has components of
//                millions of nodes, and one atomic per wave and trip on such a root serialises (components_area_kernel: 61 %
//                of a comparison's kernel time when it counted the nodes of value 0).  So a wave owns a SEGMENT of consecutive nodes and CARRIES one root in its registers: the lanes on
//                that root add to a sum of their own, which goes out with one atomic when a trip of 64 nodes holds no node of
//                the carried root (the wave then carries the root of the trip's last node) and at the segment's end.  Nodes
//                of any other root go one atomic per run of equal root.
//   count        per workgroup's chunk of nodes: the listed roots (area >= min_area); per state: all roots
//   scan/compact components.h's kernels: ids in ascending order of the roots
//   stats        per node of a listed domain with id < capacity: bounding box and distance range (atomicMin / atomicMax
//                behind a plain read), the fixed-point confidence sum, and per stored neighbour of another state one count in
//                the domain's K-bin histogram.  The same carry: box, range and sum of the carried domain in the lanes'
//                registers, its histogram in K LDS bins of the wave; other domains one atomic per run.
//   rows         per listed domain: its row of the table

#include "components.h"

namespace phmrf {
namespace {

constexpr int DOM_GRID_CAP = 1024;       // workgroups of every kernel of this file (domains.py GRID_CAP)
constexpr int DOM_EXT = 6;               // per listed domain: min i, max i, min j, max j, min d, max d

__global__ __launch_bounds__(256) void adjacency_kernel(const uint8_t* __restrict__ labels, int64_t n, int H, int W, int diagonal,
                                                        int K, unsigned long long* __restrict__ counts, int* __restrict__ bad) {
  __shared__ unsigned bins[64 * 64];
  const int nb = K * K;
  for (int t = threadIdx.x; t < nb; t += 256) bins[t] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  bool wrong = false;
  for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) - lane; base < n; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = base + lane;
    int key[4] = {-1, -1, -1, -1};
    if (v < n) {
      const int a = labels[v];
      if (a >= K) {
        wrong = true;
      } else {
        int i, j;
        grid_coords(v, W, diagonal, &i, &j);
        int64_t c[4];
        grid_forward_ids<int64_t>(v, i, j, H, W, diagonal, true, c);
#pragma unroll
        for (int d = 0; d < 4; ++d)
          if (c[d] != v) {
            const int b = labels[c[d]];
            if (b < K) key[d] = a * K + b;              // (a label >= K is reported at its own node)
          }
      }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) wave_run_add(bins, key[d], key[d] >= 0 ? 1u : 0u);
  }
  if (wrong) atomicOr(bad, 1);
  __syncthreads();
  for (int t = threadIdx.x; t < nb; t += 256)
    if (bins[t]) atomicAdd(counts + t, (unsigned long long)bins[t]);
}

// the nodes [*lo, *hi) of this wave: `seg` (a multiple of 64) consecutive nodes per wave, in wave order
__device__ __forceinline__ void wave_segment(int64_t n, int64_t seg, int64_t* lo, int64_t* hi) {
  *lo = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * seg;
  *hi = *lo + seg < n ? *lo + seg : n;
}

// Whether the wave goes on carrying `carried`: true while a lane of this trip holds it.  Otherwise the caller flushes what
// it carries and takes *next, the key of the trip's last lane with a key.  have = __ballot(key >= 0), not 0.
__device__ __forceinline__ bool carry_holds(int key, int carried, unsigned long long have, int* next) {
  if (__ballot(key == carried) & have) return true;
  *next = __shfl(key, 63 - __clzll((long long)have), 64);
  return false;
}

// acc[root] += (weight << 32) | 1 per node (weight 1 on the diagonal, 2 elsewhere), mirror[root] = 1 if j - i <= 1
__global__ __launch_bounds__(256) void domains_area_kernel(const int32_t* __restrict__ comp, int64_t n, int64_t seg, int W,
                                                           int diagonal, unsigned long long* __restrict__ acc,
                                                           uint8_t* __restrict__ mirror) {
  const int lane = threadIdx.x & 63;
  int64_t lo, hi;
  wave_segment(n, seg, &lo, &hi);
  int carried = -1;
  unsigned long long mine = 0;                         // this lane's part of the carried root
  for (int64_t base = lo; base < hi; base += 64) {
    const int64_t v = base + lane;
    int key = -1;
    unsigned long long x = 0;
    if (v < hi) {
      int i, j;
      grid_coords(v, W, diagonal, &i, &j);
      key = comp[v];
      x = ((unsigned long long)(diagonal && i == j ? 1 : 2) << 32) | 1ull;
      if (diagonal && j - i <= 1 && !mirror[key]) mirror[key] = 1;
    }
    int next;
    if (!carry_holds(key, carried, __ballot(key >= 0), &next)) {
      if (carried >= 0) wave_add(acc + carried, mine);
      mine = 0;
      carried = next;
    }
    const bool match = key >= 0 && key == carried;
    if (match) mine += x;
    wave_run_add(acc, match ? -1 : key, match ? 0ull : x);
  }
  if (carried >= 0) wave_add(acc + carried, mine);
}

// per_group[g] = listed roots among workgroup g's `chunk` consecutive nodes; ncomp[k] += its roots of state k, listed or not
__global__ __launch_bounds__(256) void domains_count_kernel(const int32_t* __restrict__ comp, const uint8_t* __restrict__ labels,
                                                            int64_t n, int64_t chunk, ListedRoot listed, int K,
                                                            int* __restrict__ per_group, unsigned long long* __restrict__ ncomp) {
  __shared__ int wave_cnt[4];
  __shared__ unsigned of_state[64];
  if (threadIdx.x < 64) of_state[threadIdx.x] = 0;
  __syncthreads();
  int64_t start, end;
  group_chunk(n, chunk, &start, &end);
  const int total = count_listed(comp, start, end, listed, wave_cnt, [&](int64_t v) { atomicAdd(of_state + labels[v], 1u); });
  if (threadIdx.x == 0) per_group[blockIdx.x] = total;
  if ((int)threadIdx.x < K && of_state[threadIdx.x]) atomicAdd(ncomp + threadIdx.x, (unsigned long long)of_state[threadIdx.x]);
}

__device__ __forceinline__ int wave_min(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int t = __shfl_down(x, off, 64);
    x = t < x ? t : x;
  }
  return x;                                            // (lane 0 holds the wave's)
}
__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int t = __shfl_down(x, off, 64);
    x = t > x ? t : x;
  }
  return x;
}

// what a lane holds of the domain its wave carries
struct Carry {
  int lo[3], hi[3];                                    // i, j, d
  unsigned long long conf;
  __device__ __forceinline__ void clear() {
    lo[0] = lo[1] = lo[2] = 0x7fffffff;
    hi[0] = hi[1] = hi[2] = -1;
    conf = 0;
  }
};

// the carried domain c goes out: one atomic per bound that gains, one for the sum, one per non-zero bin of the wave's
// histogram (bins: LDS [64] of this wave, left zeroed)
__device__ __forceinline__ void carry_flush(Carry& mine, int c, int K, unsigned* bins, int* __restrict__ ext,
                                            unsigned long long* __restrict__ hist, unsigned long long* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int lo = wave_min(mine.lo[t]), hi = wave_max(mine.hi[t]);
    if (lane == 0) widen(ext + DOM_EXT * (int64_t)c + 2 * t, lo, hi);
  }
  wave_add(sums + c, mine.conf);
  __threadfence_block();                               // (the wave's LDS atomics before its reads)
  const unsigned u = bins[lane];
  if (lane < K && u) atomicAdd(hist + (int64_t)c * K + lane, (unsigned long long)u);
  bins[lane] = 0;
  __threadfence_block();
  mine.clear();
}

// per node: domain_out[v] = the id of v's listed domain or -1; per node of a listed domain c < cap: ext[6c ..], sums[c],
// hist[c K + s] per stored neighbour of state s != the node's
__global__ __launch_bounds__(256) void domains_stats_kernel(const uint8_t* __restrict__ labels, const float* __restrict__ conf,
                                                            const int32_t* __restrict__ comp, const int32_t* __restrict__ cid,
                                                            int64_t n, int64_t seg, int H, int W, int diagonal, long long dist0,
                                                            int K, int64_t cap, int32_t* __restrict__ domain_out,
                                                            int* __restrict__ ext, unsigned long long* __restrict__ hist,
                                                            unsigned long long* __restrict__ sums) {
  __shared__ unsigned wave_bins[4][64];
  const int lane = threadIdx.x & 63;
  unsigned* bins = wave_bins[threadIdx.x >> 6];
  bins[lane] = 0;
  __threadfence_block();
  int64_t lo, hi;
  wave_segment(n, seg, &lo, &hi);
  int carried = -1;
  Carry mine;
  mine.clear();
  for (int64_t base = lo; base < hi; base += 64) {
    const int64_t v = base + lane;
    int c = -1;
    if (v < hi) {
      c = cid[comp[v]];
      if (domain_out) domain_out[v] = c;
      if (c >= cap) c = -1;
    }
    const unsigned long long have = __ballot(c >= 0);
    if (have == 0ull) continue;                        // (the same for the whole wave)
    int next;
    if (!carry_holds(c, carried, have, &next)) {
      if (carried >= 0) carry_flush(mine, carried, K, bins, ext, hist, sums);
      carried = next;
    }
    const bool match = c >= 0 && c == carried;
    int me = 0, ns[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long f = 0;
    if (c >= 0) {
      int i, j;
      grid_coords(v, W, diagonal, &i, &j);
      const long long s = dist0 + j - i;
      const int d = (int)(s < 0 ? -s : s);
      if (conf) f = (unsigned long long)(conf[v] * 16777216.0f);          // exact: a float32 in [0, 1] times 2^24
      int64_t nb[8];
      grid_neighbour_ids(v, i, j, H, W, diagonal, nb);                    // (an absent neighbour is v itself: no count)
      me = labels[v];
#pragma unroll
      for (int q = 0; q < 8; ++q) ns[q] = labels[nb[q]];
      if (match) {
        mine.lo[0] = i < mine.lo[0] ? i : mine.lo[0];
        mine.hi[0] = i > mine.hi[0] ? i : mine.hi[0];
        mine.lo[1] = j < mine.lo[1] ? j : mine.lo[1];
        mine.hi[1] = j > mine.hi[1] ? j : mine.hi[1];
        mine.lo[2] = d < mine.lo[2] ? d : mine.lo[2];
        mine.hi[2] = d > mine.hi[2] ? d : mine.hi[2];
        mine.conf += f;
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (ns[q] != me) atomicAdd(bins + ns[q], 1u);
      } else {
        int* e = ext + DOM_EXT * (int64_t)c;
        widen(e, i, i);
        widen(e + 2, j, j);
        widen(e + 4, d, d);
      }
    }
    // the nodes of the domains the wave does not carry: one atomic per run of equal destination among consecutive lanes
    const int other = match ? -1 : c;
    if (__ballot(other >= 0) == 0ull) continue;
    if (conf) wave_run_add(sums, other, other >= 0 ? f : 0ull);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int key = (other >= 0 && ns[q] != me) ? other * K + ns[q] : -1;
      if (__ballot(key >= 0) == 0ull) continue;
      wave_run_add(hist, key, key >= 0 ? 1ull : 0ull);
    }
  }
  if (carried >= 0) carry_flush(mine, carried, K, bins, ext, hist, sums);
}

__global__ __launch_bounds__(256) void domains_rows_kernel(const int32_t* __restrict__ roots, int count, int diagonal, int K,
                                                           const uint8_t* __restrict__ labels,
                                                           const unsigned long long* __restrict__ acc,
                                                           const uint8_t* __restrict__ mirror, const int* __restrict__ ext,
                                                           const unsigned long long* __restrict__ hist,
                                                           const unsigned long long* __restrict__ sums,
                                                           long long* __restrict__ table) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < count; c += gridDim.x * blockDim.x) {
    const int64_t r = roots[c];
    long long* row = table + (int64_t)c * PHMRF_STATE_DOMAIN_COLS;
    const int* e = ext + DOM_EXT * (int64_t)c;
    const Mode m = mode_of(hist + (int64_t)c * K, K);
    row[0] = r;
    row[1] = e[0];
    row[2] = e[1];
    row[3] = e[2];
    row[4] = e[3];
    row[5] = (long long)(acc[r] & 0xffffffffull);
    row[6] = component_area(r, diagonal, acc, mirror);
    row[7] = labels[r];
    row[8] = (long long)m.total;
    row[9] = m.best ? m.state : -1;      // (borders no other state)
    row[10] = (long long)m.best;
    row[11] = e[4];
    row[12] = e[5];
    row[13] = (long long)sums[c];
    row[14] = row[15] = 0;
  }
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_state_adjacency(const uint8_t* labels_dev, int H, int W, int diagonal, int K, int64_t* adj_host, void* hip_stream) {
  PHMRF_CHECK(labels_dev && adj_host, PHMRF_ERR_INVALID, "NULL buffer");
  int64_t n;
  PHMRF_TRY(check_region(H, W, diagonal, &n));
  PHMRF_TRY(check_states(K));
  PHMRF_TRY(check_nodes(n));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int nb = K * K;
  std::vector<unsigned long long> got((size_t)nb, 0ull);
  Buffers buf;
  unsigned long long* counts;
  int* flag;
  PHMRF_TRY(buf.get(&counts, (size_t)nb));
  PHMRF_TRY(buf.get(&flag, 1));
  PHMRF_HIP(hipMemsetAsync(counts, 0, (size_t)nb * sizeof(unsigned long long), st));
  PHMRF_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  hipLaunchKernelGGL(adjacency_kernel, dim3(grid_of(n, 256, DOM_GRID_CAP)), dim3(256), 0, st, labels_dev, n, H, W, diagonal, K,
                     counts, flag);
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipMemcpyAsync(got.data(), counts, (size_t)nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  PHMRF_CHECK(!bad, PHMRF_ERR_INVALID, "a label is >= K");
  // an edge was counted at (state of its first node, state of its second): both orders fold into the symmetric table
  for (int a = 0; a < K; ++a)
    for (int b = 0; b < K; ++b)
      adj_host[a * K + b] = (int64_t)(a == b ? got[(size_t)a * K + a] : got[(size_t)a * K + b] + got[(size_t)b * K + a]);
  return PHMRF_OK;
}

int phmrf_state_domains(const uint8_t* labels_dev, const float* conf_dev_or_null, int H, int W, int diagonal, int64_t dist0,
                        int K, int64_t min_area, int32_t* domain_out_dev_or_null, int64_t capacity, int64_t* table_host,
                        int64_t* n_domains, int64_t* n_components_host_or_null, void* hip_stream) {
  PHMRF_CHECK(labels_dev && n_domains, PHMRF_ERR_INVALID, "NULL buffer");
  int64_t n;
  PHMRF_TRY(check_region(H, W, diagonal, &n));
  PHMRF_TRY(check_states(K));
  PHMRF_TRY(check_nodes(n));
  PHMRF_CHECK(capacity >= 0, PHMRF_ERR_INVALID, "capacity must be >= 0");
  PHMRF_CHECK(min_area >= 1, PHMRF_ERR_INVALID, "min_area must be >= 1");
  PHMRF_CHECK(capacity == 0 || table_host, PHMRF_ERR_INVALID, "a table is needed when capacity > 0");
  PHMRF_TRY(check_reach(dist0, H, W, ""));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int g = grid_of(n, 256, DOM_GRID_CAP);
  const int64_t seg = ((n + 4 * (int64_t)g - 1) / (4 * (int64_t)g) + 63) / 64 * 64;      // areas, stats: nodes per wave
  const int64_t chunk = ((n + g - 1) / g + 255) / 256 * 256;                              // compact: nodes per workgroup

  Buffers buf;
  int* scalars;                    // [0] bad input, [1] number of listed domains
  PHMRF_TRY(buf.get(&scalars, 2));
  PHMRF_HIP(hipMemsetAsync(scalars, 0, 2 * sizeof(int), st));
  hipLaunchKernelGGL(components_check_kernel, dim3(g), dim3(256), 0, st, labels_dev, conf_dev_or_null, n, K, scalars);
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_HIP(hipMemcpyAsync(&bad, scalars, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  PHMRF_CHECK(!(bad & 1), PHMRF_ERR_INVALID, "a label is >= K");
  PHMRF_CHECK(!(bad & 2), PHMRF_ERR_INVALID, "a confidence is not a finite number in [0, 1]");

  int32_t *comp, *cid;
  unsigned long long *acc, *ncomp_dev;
  uint8_t* mirror;
  int* per_group;
  PHMRF_TRY(buf.get(&comp, (size_t)n));
  PHMRF_TRY(buf.get(&cid, (size_t)n));
  PHMRF_TRY(buf.get(&acc, (size_t)n));
  PHMRF_TRY(buf.get(&mirror, (size_t)n));
  PHMRF_TRY(buf.get(&per_group, (size_t)g));
  PHMRF_TRY(buf.get(&ncomp_dev, 64));
  const ListedRoot is_listed = {nullptr, diagonal, acc, mirror, (long long)min_area, ANY_AREA};
  PHMRF_TRY(launch_grid_components(comp, n, W, diagonal, labels_dev, st));
  PHMRF_HIP(hipMemsetAsync(acc, 0, (size_t)n * sizeof(unsigned long long), st));
  PHMRF_HIP(hipMemsetAsync(mirror, 0, (size_t)n, st));
  PHMRF_HIP(hipMemsetAsync(ncomp_dev, 0, 64 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(domains_area_kernel, dim3(g), dim3(256), 0, st, comp, n, seg, W, diagonal, acc, mirror);
  hipLaunchKernelGGL(domains_count_kernel, dim3(g), dim3(256), 0, st, comp, labels_dev, n, chunk, is_listed, K, per_group,
                     ncomp_dev);
  hipLaunchKernelGGL(components_scan_kernel, dim3(1), dim3(256), 0, st, per_group, g, scalars + 1);
  PHMRF_HIP(hipGetLastError());
  int count = 0;
  PHMRF_HIP(hipMemcpyAsync(&count, scalars + 1, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  const int64_t listed = count < capacity ? count : capacity;
  PHMRF_CHECK(listed * K < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED, "domains x states must stay below 2^31: ask for fewer rows");
  std::vector<long long> rows((size_t)listed * PHMRF_STATE_DOMAIN_COLS);
  unsigned long long ncomp[64];
  if (listed > 0 || domain_out_dev_or_null) {
    int32_t* roots;
    int* ext;
    unsigned long long *hist, *sums;
    long long* table;
    PHMRF_TRY(buf.get(&roots, (size_t)listed));
    PHMRF_TRY(buf.get(&ext, (size_t)listed * DOM_EXT));
    PHMRF_TRY(buf.get(&hist, (size_t)listed * K));
    PHMRF_TRY(buf.get(&sums, (size_t)listed));
    PHMRF_TRY(buf.get(&table, rows.size()));
    if (listed > 0) {
      PHMRF_HIP(hipMemsetAsync(hist, 0, (size_t)listed * K * sizeof(unsigned long long), st));
      PHMRF_HIP(hipMemsetAsync(sums, 0, (size_t)listed * sizeof(unsigned long long), st));
      hipLaunchKernelGGL(components_bounds_init_kernel, dim3(grid_of(listed, 256, DOM_GRID_CAP)), dim3(256), 0, st, ext,
                         (DOM_EXT / 2) * listed);
    }
    hipLaunchKernelGGL(components_compact_kernel, dim3(g), dim3(256), 0, st, comp, n, chunk, is_listed, per_group, listed, cid,
                       roots);
    hipLaunchKernelGGL(domains_stats_kernel, dim3(g), dim3(256), 0, st, labels_dev, conf_dev_or_null, comp, cid, n, seg, H, W,
                       diagonal, (long long)dist0, K, listed, domain_out_dev_or_null, ext, hist, sums);
    if (listed > 0) {
      hipLaunchKernelGGL(domains_rows_kernel, dim3(grid_of(listed, 256, DOM_GRID_CAP)), dim3(256), 0, st, roots, (int)listed,
                         diagonal, K, labels_dev, acc, mirror, ext, hist, sums, table);
      PHMRF_HIP(hipMemcpyAsync(rows.data(), table, rows.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
    }
    PHMRF_HIP(hipGetLastError());
  }
  PHMRF_HIP(hipMemcpyAsync(ncomp, ncomp_dev, sizeof(ncomp), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  for (size_t t = 0; t < rows.size(); ++t) table_host[t] = (int64_t)rows[t];
  if (n_components_host_or_null)
    for (int k = 0; k < K; ++k) n_components_host_or_null[k] = (int64_t)ncomp[k];
  *n_domains = count;
  return PHMRF_OK;
}

}  // extern "C"
