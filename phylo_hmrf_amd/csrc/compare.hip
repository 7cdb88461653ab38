// gfx950 kernels that compare two state maps of one region (phmrf_label_contingency, phmrf_diff_domains; DESIGN.md
// section 7).  Integer arithmetic throughout: no result depends on the order in which the atomics land.
//
//   contingency  counts[a, b] over the stored nodes.  Each workgroup keeps a KA x KB table of u32 bins in LDS (at most
//                16 KB) and flushes its non-zero bins with u64 global atomics.  A lane reads four nodes of either map with one
//                4-byte load where both maps can be aligned together; the run of equal (a, b) that starts a lane's four
//                goes in with ONE LDS atomic per run of equal (a, b) among consecutive lanes (wave_run_add), what is left
//                of a lane's four after a change of state goes in singly.  Heads and tails go byte-wise the same way.
//   diff         diff[v] = 0 where a == map_b[b], else 2 where the node counts (both confidences >= min_conf) and 1 where
//                it does not; the three counts per distance band |dist0 + j - i| in an LDS table per workgroup
//   components   moves.hip's union-find on the diff map (launch_grid_components); the domains are the components of value 2,
//                and they alone get the full-matrix area (components_area_kernel over the nodes of value 2, components.h)
//   compact      roots of value 2 with area >= min_area get consecutive ids in node order (components.h's count, scan and
//                compact kernels: a chunk of nodes per workgroup, the workgroups' offsets from a scan) and are listed in that
//                order
//   stats        per node of a listed domain: bounding box by atomicMin / atomicMax, the two K-bin u64 state histograms
//                and the two fixed-point confidence sums, one atomic per run of equal destination among consecutive lanes
//   rows         per listed domain: its row of the table

#include "components.h"

#include <cstring>

namespace phmrf {
namespace {

constexpr int CONT_GRID_CAP = 1024;      // workgroups of the contingency kernel (compare.py CONTINGENCY_GRID_CAP)
constexpr int CONT_PER_TRIP = 1024;      // nodes a workgroup reads per grid-stride trip: 256 lanes x 4 bytes

// Nodes [0, head) and [tail, n) go byte-wise, the nvec 4-byte words between them as words; bins: LDS [KA * KB]
__global__ __launch_bounds__(256) void contingency_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                          int64_t n, int64_t head, int64_t nvec, int KA, int KB,
                                                          unsigned long long* __restrict__ counts, int* __restrict__ bad) {
  __shared__ unsigned bins[64 * 64];
  const int nb = KA * KB;
  for (int t = threadIdx.x; t < nb; t += 256) bins[t] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) - lane, stride = (int64_t)gridDim.x * blockDim.x;
  bool wrong = false;
  const uint32_t* __restrict__ a4 = reinterpret_cast<const uint32_t*>(a + head);
  const uint32_t* __restrict__ b4 = reinterpret_cast<const uint32_t*>(b + head);
  for (int64_t base = first; base < nvec; base += stride) {
    const int64_t u = base + lane;
    int key[4] = {-1, -1, -1, -1};
    if (u < nvec) {
      const uint32_t wa = a4[u], wb = b4[u];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int sa = (wa >> (8 * e)) & 0xff, sb = (wb >> (8 * e)) & 0xff;
        if (sa < KA && sb < KB) key[e] = sa * KB + sb;
        else wrong = true;
      }
    }
    wave_quad_add(bins, key);                            // the run of equal (a, b) that starts the lane's four, the rest singly
  }
  const int64_t tail = head + 4 * nvec, nbytes = head + (n - tail);
  for (int64_t base = first; base < nbytes; base += stride) {
    const int64_t q = base + lane;
    int key = -1;
    if (q < nbytes) {
      const int64_t v = q < head ? q : tail + (q - head);
      const int sa = a[v], sb = b[v];
      if (sa < KA && sb < KB) key = sa * KB + sb;
      else wrong = true;
    }
    wave_run_add(bins, key, key >= 0 ? 1u : 0u);
  }
  if (wrong) atomicOr(bad, 1);
  __syncthreads();
  for (int t = threadIdx.x; t < nb; t += 256)
    if (bins[t]) atomicAdd(counts + t, (unsigned long long)bins[t]);
}

struct MapB {
  uint8_t to[64];
};

// diff[v] and the band counts; bad |= 1 for a label >= K, 2 for a confidence that is not a finite number in [0, 1]
__global__ __launch_bounds__(256) void compare_diff_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, MapB map,
                                                           const float* __restrict__ conf_a, const float* __restrict__ conf_b,
                                                           int64_t n, int W, int diagonal, long long dist0, int KA, int KB,
                                                           float min_conf, uint8_t* __restrict__ diff,
                                                           unsigned long long* __restrict__ bands, int* __restrict__ bad) {
  __shared__ unsigned tab[PHMRF_DIFF_BANDS * 3];
  if (threadIdx.x < PHMRF_DIFF_BANDS * 3) tab[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  int wrong = 0;
  for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) - lane; base < n; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = base + lane;
    int band = -1, d = 0;
    if (v < n) {
      const int sa = a[v], sb = b[v];
      if (sa >= KA || sb >= KB) {
        wrong |= 1;
      } else if (sa != (int)map.to[sb]) {
        d = 2;
        if (conf_a) {
          const float ca = conf_a[v], cb = conf_b[v];
          if (!unit_conf(ca) || !unit_conf(cb)) wrong |= 2;
          else if (min_conf > 0.0f && !(ca >= min_conf && cb >= min_conf)) d = 1;
        }
      } else if (conf_a) {
        if (!unit_conf(conf_a[v]) || !unit_conf(conf_b[v])) wrong |= 2;
      }
      diff[v] = (uint8_t)d;
      int i, j;
      grid_coords(v, W, diagonal, &i, &j);
      const long long s = dist0 + j - i;
      band = band_of(s < 0 ? -s : s);
    }
    // one LDS atomic per count and run of equal band among consecutive lanes
    wave_run_add(tab, band >= 0 ? 3 * band : -1, band >= 0 ? 1u : 0u);
    wave_run_add(tab, band >= 0 ? 3 * band + 1 : -1, d >= 1 ? 1u : 0u);
    wave_run_add(tab, band >= 0 ? 3 * band + 2 : -1, d == 2 ? 1u : 0u);
  }
  if (wrong) atomicOr(bad, wrong);
  __syncthreads();
  if (threadIdx.x < PHMRF_DIFF_BANDS * 3 && tab[threadIdx.x]) atomicAdd(bands + threadIdx.x, (unsigned long long)tab[threadIdx.x]);
}

// per node of a listed domain c < cap: box[4c ..] = min i, max i, min j, max j; hist_a[c KA + a], hist_b[c KM + map[b]],
// sums[2c], sums[2c + 1] the fixed-point confidences
__global__ __launch_bounds__(256) void compare_stats_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, MapB map,
                                                            const float* __restrict__ conf_a, const float* __restrict__ conf_b,
                                                            const uint8_t* __restrict__ diff, const int32_t* __restrict__ comp,
                                                            const int32_t* __restrict__ cid, int64_t n, int W, int diagonal,
                                                            int KA, int KM, int64_t cap, int* __restrict__ box,
                                                            unsigned long long* __restrict__ hist_a,
                                                            unsigned long long* __restrict__ hist_b,
                                                            unsigned long long* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) - lane; base < n; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = base + lane;
    int c = -1;
    if (v < n && diff[v] == 2) {
      c = cid[comp[v]];
      if (c >= cap) c = -1;
    }
    if (__ballot(c >= 0) == 0ull) continue;             // (the same for the whole wave)
    int ka = -1, kb = -1;
    unsigned long long fa = 0, fb = 0;
    if (c >= 0) {
      int i, j;
      grid_coords(v, W, diagonal, &i, &j);
      widen(box + 4 * (int64_t)c, i, i);
      widen(box + 4 * (int64_t)c + 2, j, j);
      ka = c * KA + a[v];
      kb = c * KM + map.to[b[v]];
      if (conf_a) {
        fa = (unsigned long long)(conf_a[v] * 16777216.0f);        // exact: a float32 in [0, 1] times 2^24
        fb = (unsigned long long)(conf_b[v] * 16777216.0f);
      }
    }
    wave_run_add(hist_a, ka, c >= 0 ? 1ull : 0ull);
    wave_run_add(hist_b, kb, c >= 0 ? 1ull : 0ull);
    if (conf_a) {
      wave_run_add(sums, c >= 0 ? 2 * c : -1, fa);
      wave_run_add(sums, c >= 0 ? 2 * c + 1 : -1, fb);
    }
  }
}

__global__ __launch_bounds__(256) void compare_rows_kernel(const int32_t* __restrict__ roots, int count, int diagonal,
                                                           const unsigned long long* __restrict__ acc,
                                                           const uint8_t* __restrict__ mirror, const int* __restrict__ box,
                                                           const unsigned long long* __restrict__ hist_a,
                                                           const unsigned long long* __restrict__ hist_b,
                                                           const unsigned long long* __restrict__ sums, int KA, int KM,
                                                           long long* __restrict__ table) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < count; c += gridDim.x * blockDim.x) {
    const int64_t r = roots[c];
    long long* row = table + (int64_t)c * PHMRF_DOMAIN_COLS;
    row[0] = r;
    row[1] = box[4 * (int64_t)c];
    row[2] = box[4 * (int64_t)c + 1];
    row[3] = box[4 * (int64_t)c + 2];
    row[4] = box[4 * (int64_t)c + 3];
    row[5] = (long long)(acc[r] & 0xffffffffull);
    row[6] = component_area(r, diagonal, acc, mirror);
    row[7] = mode_of(hist_a + (int64_t)c * KA, KA).state;
    row[8] = mode_of(hist_b + (int64_t)c * KM, KM).state;
    row[9] = (long long)sums[2 * (int64_t)c];
    row[10] = (long long)sums[2 * (int64_t)c + 1];
    row[11] = 0;
  }
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_label_contingency(const uint8_t* a_dev, const uint8_t* b_dev, int64_t n, int KA, int KB, int64_t* counts_host,
                            void* hip_stream) {
  PHMRF_CHECK(a_dev && b_dev && counts_host, PHMRF_ERR_INVALID, "NULL buffer");
  PHMRF_CHECK(n >= 0, PHMRF_ERR_INVALID, "n must be >= 0");
  PHMRF_TRY(check_states(KA, KB, "KA and KB"));
  PHMRF_TRY(check_nodes(n, "n must be below 2^31 - 64"));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int nb = KA * KB;
  std::vector<unsigned long long> got((size_t)nb, 0ull);
  if (n > 0) {
    // words where both maps are 4-byte aligned at the same node; otherwise every node goes byte-wise
    int64_t head = (int64_t)((4 - (reinterpret_cast<uintptr_t>(a_dev) & 3)) & 3);
    if (head > n) head = n;
    const bool together = ((reinterpret_cast<uintptr_t>(b_dev) + (uintptr_t)head) & 3) == 0;
    const int64_t nvec = together ? (n - head) / 4 : 0;
    if (!together) head = 0;
    Buffers buf;
    unsigned long long* counts;
    int* flag;
    PHMRF_TRY(buf.get(&counts, (size_t)nb));
    PHMRF_TRY(buf.get(&flag, 1));
    PHMRF_HIP(hipMemsetAsync(counts, 0, (size_t)nb * sizeof(unsigned long long), st));
    PHMRF_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    const int g = grid_of(n, CONT_PER_TRIP, CONT_GRID_CAP);
    hipLaunchKernelGGL(contingency_kernel, dim3(g), dim3(256), 0, st, a_dev, b_dev, n, head, nvec, KA, KB, counts, flag);
    PHMRF_HIP(hipGetLastError());
    int bad = 0;
    PHMRF_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    PHMRF_HIP(hipMemcpyAsync(got.data(), counts, (size_t)nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    PHMRF_HIP(hipStreamSynchronize(st));
    PHMRF_CHECK(!bad, PHMRF_ERR_INVALID, "a label is >= K");
  }
  for (int t = 0; t < nb; ++t) counts_host[t] = (int64_t)got[t];
  return PHMRF_OK;
}

int phmrf_diff_domains(const uint8_t* a_dev, const uint8_t* b_dev, const uint8_t* map_b_host_or_null,
                       const float* conf_a_dev_or_null, const float* conf_b_dev_or_null, int H, int W, int diagonal,
                       int64_t dist0, int KA, int KB, float min_conf, int64_t min_area, uint8_t* diff_out_dev_or_null,
                       int64_t capacity, int64_t* table_host, int64_t* n_domains, int64_t* band_counts_host_or_null,
                       void* hip_stream) {
  PHMRF_CHECK(a_dev && b_dev && n_domains, PHMRF_ERR_INVALID, "NULL buffer");
  PHMRF_CHECK((conf_a_dev_or_null == nullptr) == (conf_b_dev_or_null == nullptr), PHMRF_ERR_INVALID,
              "give both confidences or neither");
  int64_t n;
  PHMRF_TRY(check_region(H, W, diagonal, &n));
  PHMRF_TRY(check_states(KA, KB, "KA and KB"));
  PHMRF_CHECK(capacity >= 0, PHMRF_ERR_INVALID, "capacity must be >= 0");
  PHMRF_CHECK(min_area >= 1, PHMRF_ERR_INVALID, "min_area must be >= 1");
  PHMRF_CHECK(capacity == 0 || table_host, PHMRF_ERR_INVALID, "a table is needed when capacity > 0");
  uint32_t mc_bits;
  std::memcpy(&mc_bits, &min_conf, sizeof(mc_bits));
  PHMRF_CHECK((mc_bits & 0x7fffffffu) <= 0x7f800000u, PHMRF_ERR_INVALID, "min_conf is not a number");
  PHMRF_TRY(check_reach(dist0, H, W));
  MapB map;
  int KM = KB;
  for (int k = 0; k < 64; ++k) map.to[k] = (uint8_t)k;
  if (map_b_host_or_null) {
    KM = 1;
    for (int k = 0; k < KB; ++k) {
      PHMRF_CHECK(map_b_host_or_null[k] < 64, PHMRF_ERR_INVALID, "map_b values must be < 64");
      map.to[k] = map_b_host_or_null[k];
      if (map.to[k] + 1 > KM) KM = map.to[k] + 1;
    }
  }
  PHMRF_TRY(check_nodes(n));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int g = grid_of(n);
  const int64_t chunk = ((n + g - 1) / g + 255) / 256 * 256;     // compact: consecutive nodes per workgroup

  Buffers buf;
  int* scalars;                    // [0] bad input, [1] number of listed domains
  unsigned long long* bands_dev;
  uint8_t* diff;
  PHMRF_TRY(buf.get(&scalars, 2));
  PHMRF_TRY(buf.get(&bands_dev, (size_t)PHMRF_DIFF_BANDS * 3));
  PHMRF_TRY(buf.get(&diff, (size_t)n));
  PHMRF_HIP(hipMemsetAsync(scalars, 0, 2 * sizeof(int), st));
  PHMRF_HIP(hipMemsetAsync(bands_dev, 0, (size_t)PHMRF_DIFF_BANDS * 3 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(compare_diff_kernel, dim3(g), dim3(256), 0, st, a_dev, b_dev, map, conf_a_dev_or_null, conf_b_dev_or_null,
                     n, W, diagonal, (long long)dist0, KA, KB, min_conf, diff, bands_dev, scalars);
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_HIP(hipMemcpyAsync(&bad, scalars, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  PHMRF_CHECK(!(bad & 1), PHMRF_ERR_INVALID, "a label is >= K");
  PHMRF_CHECK(!(bad & 2), PHMRF_ERR_INVALID, "a confidence is not a finite number in [0, 1]");

  int32_t *comp, *cid;
  unsigned long long* acc;
  uint8_t* mirror;
  int* per_group;
  PHMRF_TRY(buf.get(&comp, (size_t)n));
  PHMRF_TRY(buf.get(&cid, (size_t)n));
  PHMRF_TRY(buf.get(&acc, (size_t)n));
  PHMRF_TRY(buf.get(&mirror, (size_t)n));
  PHMRF_TRY(buf.get(&per_group, (size_t)g));
  const ListedRoot is_listed = {diff, diagonal, acc, mirror, (long long)min_area, ANY_AREA};
  PHMRF_TRY(launch_grid_components(comp, n, W, diagonal, diff, st));
  PHMRF_HIP(hipMemsetAsync(acc, 0, (size_t)n * sizeof(unsigned long long), st));
  PHMRF_HIP(hipMemsetAsync(mirror, 0, (size_t)n, st));
  hipLaunchKernelGGL(components_area_kernel<DiffNode>, dim3(g), dim3(256), 0, st, comp, DiffNode{diff}, n, W, diagonal, acc, mirror);
  hipLaunchKernelGGL(components_count_kernel, dim3(g), dim3(256), 0, st, comp, n, chunk, is_listed, per_group);
  hipLaunchKernelGGL(components_scan_kernel, dim3(1), dim3(256), 0, st, per_group, g, scalars + 1);
  PHMRF_HIP(hipGetLastError());
  int count = 0;
  PHMRF_HIP(hipMemcpyAsync(&count, scalars + 1, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  const int64_t listed = count < capacity ? count : capacity;
  PHMRF_CHECK(listed * (KA > KM ? KA : KM) < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED,
              "domains x states must stay below 2^31: ask for fewer rows");
  std::vector<long long> rows((size_t)listed * PHMRF_DOMAIN_COLS);
  if (listed > 0) {
    int32_t* roots;
    int* box;
    unsigned long long *hist_a, *hist_b, *sums;
    long long* table;
    PHMRF_TRY(buf.get(&roots, (size_t)listed));
    PHMRF_TRY(buf.get(&box, (size_t)listed * 4));
    PHMRF_TRY(buf.get(&hist_a, (size_t)listed * KA));
    PHMRF_TRY(buf.get(&hist_b, (size_t)listed * KM));
    PHMRF_TRY(buf.get(&sums, (size_t)listed * 2));
    PHMRF_TRY(buf.get(&table, rows.size()));
    PHMRF_HIP(hipMemsetAsync(hist_a, 0, (size_t)listed * KA * sizeof(unsigned long long), st));
    PHMRF_HIP(hipMemsetAsync(hist_b, 0, (size_t)listed * KM * sizeof(unsigned long long), st));
    PHMRF_HIP(hipMemsetAsync(sums, 0, (size_t)listed * 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(components_bounds_init_kernel, dim3(grid_of(listed)), dim3(256), 0, st, box, 2 * listed);
    hipLaunchKernelGGL(components_compact_kernel, dim3(g), dim3(256), 0, st, comp, n, chunk, is_listed, per_group, listed, cid,
                       roots);
    hipLaunchKernelGGL(compare_stats_kernel, dim3(g), dim3(256), 0, st, a_dev, b_dev, map, conf_a_dev_or_null,
                       conf_b_dev_or_null, diff, comp, cid, n, W, diagonal, KA, KM, listed, box, hist_a, hist_b, sums);
    hipLaunchKernelGGL(compare_rows_kernel, dim3(grid_of(listed)), dim3(256), 0, st, roots, (int)listed, diagonal, acc, mirror,
                       box, hist_a, hist_b, sums, KA, KM, table);
    PHMRF_HIP(hipGetLastError());
    PHMRF_HIP(hipMemcpyAsync(rows.data(), table, rows.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
  }
  unsigned long long bands[PHMRF_DIFF_BANDS * 3];
  PHMRF_HIP(hipMemcpyAsync(bands, bands_dev, sizeof(bands), hipMemcpyDeviceToHost, st));
  if (diff_out_dev_or_null) PHMRF_HIP(hipMemcpyAsync(diff_out_dev_or_null, diff, (size_t)n, hipMemcpyDeviceToDevice, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  for (size_t t = 0; t < rows.size(); ++t) table_host[t] = (int64_t)rows[t];
  if (band_counts_host_or_null)
    for (int t = 0; t < PHMRF_DIFF_BANDS * 3; ++t) band_counts_host_or_null[t] = (int64_t)bands[t];
  *n_domains = count;
  return PHMRF_OK;
}

}  // extern "C"
