// gfx950 kernels that profile the states of a block's labelling (phmrf_state_hist, phmrf_state_moments; DESIGN.md
// section 7) over the nodes the block OWNS.  Everything but the two floating-point sums is integer arithmetic.
//
//   hist      one pass of a radix selection on the orderable key of the f32 observations.  A workgroup handles one
//             (species, slot) pair -- blockIdx.y = s * J + j -- with a [K][256] table of u32 bins in LDS (dynamic: 1 KB per
//             state, 64 KB at K = 64) and flushes its non-zero bins with one u64 global atomic each.  Within a state most
//             values of a species share their top byte and often the second, so a wave's lanes mostly hit one bin: the first
//             HIST_LEADERS distinct (state, digit) pairs of a wave go in with ONE LDS atomic each (a leader adds the number of
//             lanes that share its bin), whatever is left after that is spread over many bins and goes in lane by lane.
//   moments   count, sum x, sum x^2 per state (and species) and the distance-band counts, in one pass.  One wave per
//             workgroup.  The counts go through u32 LDS bins, one atomic per run of equal destination among consecutive lanes
//             (wave_run_add).  The sums are doubles and never meet an atomic: a segmented prefix sum over the runs of equal
//             state among the wave's lanes, each run's last lane adds the run's part to the workgroup's LDS table, run after
//             run in lane order; every workgroup stores its table as a row of partials and a second kernel adds the rows in
//             a fixed order.  The grid depends on the node count, K and S alone, so two calls add in the same order and return
//             the same bytes -- with PHMRF_DETERMINISTIC or without: there is no other path.

#include "runs.h"

#include <algorithm>

namespace phmrf {
namespace {

constexpr int HIST_GRID_CAP = 512;       // workgroups along x of the histogram kernel (profile.py HIST_GRID_CAP): at most
                                         // 2^31 / 512 = 2^22 nodes per workgroup, so no u32 bin can overflow
constexpr int HIST_LEADERS = 4;          // distinct bins of a wave that go in aggregated before the lanes go in singly
constexpr int MOM_GRID_CAP = 8192;       // workgroups (of one wave) of the moments kernel = rows of partial sums: 32 waves a CU
constexpr int MOM_PARTIAL_CAP = 1 << 22; //   ... and at most this many doubles of partial sums (32 MB: 2,048 rows at K = 64, S = 16)

extern __shared__ __attribute__((aligned(16))) char profile_lds[];

// the orderable key of an f32 bit pattern: ascending unsigned keys are ascending floats, -0 below +0, the non-finite
// patterns at the two ends
__device__ __forceinline__ uint32_t order_key(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }

// hist[((k S + s) J + j) 256 + digit] += 1 per node of [first, last) with label k whose key matches prefix[(k S + s) J + j]
// above the digit at `shift` (shift == 24: every node).  LDS: K * 256 bins -- all of the 64 KB a launch gets without asking
// for more at K = 64, so the K prefixes a workgroup needs stay in global memory (a cached load per node).
__global__ __launch_bounds__(256) void state_hist_kernel(const float* __restrict__ X, const uint8_t* __restrict__ labels,
                                                         int64_t first, int64_t last, int S, int K, int J, int shift,
                                                         const uint32_t* __restrict__ prefix,
                                                         unsigned long long* __restrict__ hist) {
  unsigned* bins = reinterpret_cast<unsigned*>(profile_lds);
  const int s = blockIdx.y / J, j = blockIdx.y - s * J;
  const int nb = K * 256;
  for (int t = threadIdx.x; t < nb; t += 256) bins[t] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int above = shift + 8;
  for (int64_t base = first + ((int64_t)blockIdx.x * 256 + threadIdx.x) - lane; base < last; base += (int64_t)gridDim.x * 256) {
    const int64_t v = base + lane;
    int bin = -1;
    if (v < last) {
      const int k = labels[v];
      if (k < K) {
        const uint32_t key = order_key(__float_as_uint(X[v * S + s]));
        if (shift == 24 || (key >> above) == prefix[((int64_t)k * S + s) * J + j]) bin = k * 256 + (int)((key >> shift) & 255u);
      }
    }
    unsigned long long pending = __ballot(bin >= 0);                 // (the same for the whole wave, as the loop below)
    for (int it = 0; it < HIST_LEADERS && pending; ++it) {
      const int leader = __ffsll((long long)pending) - 1;
      const int lb = __shfl(bin, leader, 64);
      const unsigned long long same = __ballot(bin == lb);
      if (lane == leader) atomicAdd(bins + lb, (unsigned)__popcll(same));
      if (bin == lb) bin = -1;
      pending &= ~same;
    }
    if (bin >= 0) atomicAdd(bins + bin, 1u);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nb; t += 256)
    if (bins[t]) atomicAdd(hist + (((int64_t)(t >> 8) * S + s) * J + j) * 256 + (t & 255), (unsigned long long)bins[t]);
}

// One wave per workgroup over the nodes [first, last).  partial[blockIdx.x][k][s][2] = the workgroup's (sum x, sum x^2);
// count[k], bands[k * 32 + band] (bands == NULL: skipped) += the workgroup's counts.
// LDS: K * 2 S doubles, K u32 counts, K * PHMRF_DIFF_BANDS u32 band counts.
__global__ __launch_bounds__(64) void state_moments_kernel(const float* __restrict__ X, const uint8_t* __restrict__ labels,
                                                           int64_t first, int64_t last, int S, int K, int W, int diagonal,
                                                           long long dist0, double* __restrict__ partial,
                                                           unsigned long long* __restrict__ count,
                                                           unsigned long long* __restrict__ bands) {
  const int M = K * 2 * S;
  double* part = reinterpret_cast<double*>(profile_lds);
  unsigned* cnt = reinterpret_cast<unsigned*>(part + M);
  unsigned* bnd = cnt + K;
  const int lane = threadIdx.x;
  for (int t = lane; t < M; t += 64) part[t] = 0.0;
  for (int t = lane; t < K * (1 + PHMRF_DIFF_BANDS); t += 64) cnt[t] = 0;      // (cnt and bnd are one stretch)
  __syncthreads();
  double2* acc = reinterpret_cast<double2*>(part);      // (sum x, sum x^2) of a (state, species): one 16-byte access
  for (int64_t base = first + (int64_t)blockIdx.x * 64; base < last; base += (int64_t)gridDim.x * 64) {
    const int64_t v = base + lane;
    int k = -1;
    if (v < last) {
      k = labels[v];
      if (k >= K) k = -1;
    }
    const int k_prev = __shfl_up(k, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || k_prev != k);
    const int h = 63 - __clzll((long long)(heads & lanes_at_or_below(lane)));   // the first lane of this lane's run
    const bool last_of_run = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    const unsigned long long tails = __ballot(last_of_run && k >= 0);
    wave_run_add(cnt, k, k >= 0 ? 1u : 0u);
    if (bands) {
      int key = -1;
      if (k >= 0) {
        int i, j;
        grid_coords(v, W, diagonal, &i, &j);
        const long long d = dist0 + j - i;
        key = k * PHMRF_DIFF_BANDS + band_of(d < 0 ? -d : d);
      }
      wave_run_add(bnd, key, key >= 0 ? 1u : 0u);
    }
    for (int s = 0; s < S; ++s) {
      double x = k >= 0 ? (double)X[v * S + s] : 0.0;
      double q = x * x;                 // exact: the square of an f32 fits a double
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {                       // segmented inclusive prefix sums over the runs
        const double tx = __shfl_up(x, off, 64), tq = __shfl_up(q, off, 64);
        if (lane - off >= h) {
          x += tx;
          q += tq;
        }
      }
      for (unsigned long long m = tails; m; m &= m - 1) {             // run after run: two runs may share a state
        if (lane == __ffsll((long long)m) - 1) {
          double2 a = acc[k * S + s];
          a.x += x;
          a.y += q;
          acc[k * S + s] = a;
        }
        // the runs' adds happen one after the other, as written: the compiler may not move an access across this line, and
        // the LDS serves a wave's accesses in the order they were issued
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  __syncthreads();
  for (int t = lane; t < M; t += 64) partial[(int64_t)blockIdx.x * M + t] = part[t];
  for (int t = lane; t < K; t += 64)
    if (cnt[t]) atomicAdd(count + t, (unsigned long long)cnt[t]);
  if (bands)
    for (int t = lane; t < K * PHMRF_DIFF_BANDS; t += 64)
      if (bnd[t]) atomicAdd(bands + t, (unsigned long long)bnd[t]);
}

// out[t] = the sum over the rows of partial[row][t], t = blockIdx.x: thread r adds the rows r, r + 256, ... in that order, the
// 256 parts are then added pairwise in a fixed tree.  (One thread per t walking all rows took 0.75 ms for 2,048 rows --
// every add waiting for its load --, more than the pass over 12 M nodes before it.)
__global__ __launch_bounds__(256) void state_moments_reduce_kernel(const double* __restrict__ partial, int rows, int M,
                                                                   double* __restrict__ out) {
  __shared__ double part[256];
  const int t = blockIdx.x;
  double a = 0.0;
  for (int g = threadIdx.x; g < rows; g += 256) a += partial[(int64_t)g * M + t];
  part[threadIdx.x] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[t] = part[0];
}

int owned_range(const phmrf_block* b, int64_t* first, int64_t* last) {
  PHMRF_CHECK(b->has_X, PHMRF_ERR_STATE, "observations not set");
  PHMRF_CHECK(b->has_labels, PHMRF_ERR_STATE, "labels not set (phmrf_block_set_labels or a solve)");
  *first = b->own1 >= 0 ? b->own0 : 0;
  *last = b->own1 >= 0 ? b->own1 : b->n;
  return PHMRF_OK;
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_state_hist(phmrf_block_t b, int shift, int J, const uint32_t* prefix, uint64_t* hist) {
  PHMRF_CHECK(b && hist, PHMRF_ERR_INVALID, "NULL argument");
  PHMRF_CHECK(shift == 24 || shift == 16 || shift == 8 || shift == 0, PHMRF_ERR_INVALID, "shift must be 24, 16, 8 or 0");
  PHMRF_CHECK(J >= 1 && J <= 16, PHMRF_ERR_INVALID, "J must be in [1,16]");
  PHMRF_CHECK(shift != 24 || J == 1, PHMRF_ERR_INVALID, "the first pass (shift 24) has one slot: J must be 1");
  PHMRF_CHECK(shift == 24 || prefix, PHMRF_ERR_INVALID, "a pass below the top byte needs its prefixes");
  int64_t first, last;
  PHMRF_TRY(owned_range(b, &first, &last));
  const int K = b->K, S = b->S;
  const size_t slots = (size_t)K * S * J, nbins = slots * 256;
  Buffers buf;
  uint32_t* prefix_dev;
  unsigned long long* hist_dev;
  PHMRF_TRY(buf.get(&prefix_dev, slots));
  PHMRF_TRY(buf.get(&hist_dev, nbins));
  if (shift != 24) PHMRF_HIP(hipMemcpyAsync(prefix_dev, prefix, slots * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
  PHMRF_HIP(hipMemsetAsync(hist_dev, 0, nbins * sizeof(unsigned long long), b->stream));
  if (last > first) {
    const dim3 grid(grid_of(last - first, 256, HIST_GRID_CAP), S * J);
    const size_t lds = (size_t)K * 256 * sizeof(unsigned);
    hipLaunchKernelGGL(state_hist_kernel, grid, dim3(256), lds, b->stream, b->X, b->labels, first, last, S, K, J, shift, prefix_dev,
                       hist_dev);
    PHMRF_HIP(hipGetLastError());
  }
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the bins are read back as they are");
  PHMRF_HIP(hipMemcpyAsync(hist, hist_dev, nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  return PHMRF_OK;
}

int phmrf_state_moments(phmrf_block_t b, int64_t dist0, int64_t* count, double* sum, double* sumsq, int64_t* bands_or_null) {
  PHMRF_CHECK(b && count && sum && sumsq, PHMRF_ERR_INVALID, "NULL argument");
  int64_t first, last;
  PHMRF_TRY(owned_range(b, &first, &last));
  if (bands_or_null) {
    PHMRF_CHECK(b->has_grid, PHMRF_ERR_STATE, "distance bands need the grid geometry (phmrf_block_set_grid / build_grid_graph)");
    PHMRF_TRY(check_reach(dist0, b->H, b->W));
  }
  const int K = b->K, S = b->S, M = K * 2 * S, NC = K * (1 + PHMRF_DIFF_BANDS);
  const int rows = grid_of(last - first, 64, std::min(MOM_GRID_CAP, MOM_PARTIAL_CAP / M));
  Buffers buf;
  double *partial, *sums_dev;
  unsigned long long* counts;                // [K] counts, then [K * 32] bands
  PHMRF_TRY(buf.get(&partial, (size_t)rows * M));
  PHMRF_TRY(buf.get(&sums_dev, (size_t)M));
  PHMRF_TRY(buf.get(&counts, (size_t)NC));
  PHMRF_HIP(hipMemsetAsync(counts, 0, (size_t)NC * sizeof(unsigned long long), b->stream));
  PHMRF_HIP(hipMemsetAsync(sums_dev, 0, (size_t)M * sizeof(double), b->stream));
  if (last > first) {
    const size_t lds = (size_t)M * sizeof(double) + (size_t)NC * sizeof(unsigned);
    hipLaunchKernelGGL(state_moments_kernel, dim3(rows), dim3(64), lds, b->stream, b->X, b->labels, first, last, S, K, b->W,
                       b->diagonal, (long long)dist0, partial, counts, bands_or_null ? counts + K : nullptr);
    hipLaunchKernelGGL(state_moments_reduce_kernel, dim3(M), dim3(256), 0, b->stream, partial, rows, M, sums_dev);
    PHMRF_HIP(hipGetLastError());
  }
  std::vector<unsigned long long> got((size_t)NC);
  std::vector<double> sums((size_t)M);
  PHMRF_HIP(hipMemcpyAsync(got.data(), counts, (size_t)NC * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipMemcpyAsync(sums.data(), sums_dev, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  PHMRF_HIP(hipStreamSynchronize(b->stream));
  for (int k = 0; k < K; ++k) count[k] = (int64_t)got[k];
  for (int t = 0; t < K * S; ++t) {
    sum[t] = sums[2 * t];
    sumsq[t] = sums[2 * t + 1];
  }
  if (bands_or_null)
    for (int t = 0; t < K * PHMRF_DIFF_BANDS; ++t) bands_or_null[t] = (int64_t)got[K + t];
  return PHMRF_OK;
}

}  // extern "C"
