// gfx950 kernels of the raw loader's smoothing filters (preprocess.py `_apply_filter`): the device
// halves of preprocess.anisotropic_diffusion (filter_mode 0), preprocess_host.cpp's phmrf_bilateral (filter_mode 1) and
// scipy.ndimage.gaussian_filter (any other mode with sigma > 0).  No block: every call works on ONE H x W plane in device
// memory, is queued on the caller's stream and returns when done.
//
//   diffusion   one launch per Perona-Malik step, ping-pong between the image and a scratch plane.  A pixel reads its four
//               neighbours and recomputes the two fluxes it shares with its north and west neighbours (4 exp per pixel)
//               rather than storing flux planes: 8 B of HBM traffic per pixel and step.  float32 throughout, true division,
//               no FMA contraction, so that every operation is the one NumPy's float32 arrays round; with that the step is
//               bound by its vector instructions (0.22 of the HBM peak at 4,979^2), and by its copies as the loader uses it.
//   bilateral   a workgroup of 1024 threads owns a 64 x 64 output tile and stages the tile plus its halo, zero outside the
//               image, in LDS ((63 + win)^2 doubles: 69 KB at win = 31) beside the colour table (80 KB at 10,000 bins).  A
//               thread owns 4 consecutive rows of one column: it walks the 3 + win halo rows that feed them once, row by row
//               and column by column, so a halo value is read once for up to 4 outputs and every output still adds its taps
//               in the host's order (window row, then window column).  The tap of a step is the same in every lane: the
//               spatial weight is a wave-uniform load.  A wave reads 64 consecutive doubles of one halo row (no bank
//               conflict); the colour-table gather is the one irregular access: from LDS 7.0 ms at 4,979^2 pixels and
//               window 31 on an MI355X, from global memory (L2) 24.6 ms (-DPHMRF_BILATERAL_LUT_GLOBAL builds that).  Tables
//               that do not fit (a window above 37 with the table, above 79 alone; more than ~11,000 bins) fall back to
//               global memory, tile first.
//   gaussian    two separable passes (axis 0 into the scratch plane, axis 1 into the output) with scipy's symmetric
//               correlation order and its `reflect` border, the weights computed on the host.

#include <algorithm>
#include <cmath>

#include "runs.h"

namespace phmrf {
namespace {

// the launches below tile the plane with 64-column workgroups and stride over the rows
constexpr int ROWS_PER_WG = 4;
inline dim3 plane_grid(int64_t H, int64_t W) {
  const int64_t gx = (W + 63) / 64;
  int64_t gy = (H + ROWS_PER_WG - 1) / ROWS_PER_WG;
  const int64_t cap = std::max<int64_t>(1, 16384 / gx);
  if (gy > cap) gy = cap;
  return dim3((unsigned)gx, (unsigned)gy);
}

// ---- diffusion ------------------------------------------------------------------------------------------------------
template <int OPTION>
__device__ __forceinline__ float pm_flux(float d, float kappa) {
#pragma clang fp contract(off)
  const float t = d / kappa;
  const float c = OPTION == 1 ? expf(-(t * t)) : 1.0f / (1.0f + t * t);
  return c * d;
}

template <int OPTION>
__global__ __launch_bounds__(256) void diffusion_step_kernel(const float* __restrict__ in, float* __restrict__ out, int H,
                                                             int W, float kappa, float gamma) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= W) return;
  for (int i = blockIdx.y * ROWS_PER_WG + threadIdx.y; i < H; i += gridDim.y * ROWS_PER_WG) {
    const int64_t q = (int64_t)i * W + j;
    const float c = in[q];
    // forward differences are 0 at the far border; row / column 0 keeps its own flux (np.diff leaves flux[0])
    const float fs = i + 1 < H ? pm_flux<OPTION>(in[q + W] - c, kappa) : 0.0f;
    const float fe = j + 1 < W ? pm_flux<OPTION>(in[q + 1] - c, kappa) : 0.0f;
    const float ds = i > 0 ? fs - pm_flux<OPTION>(c - in[q - W], kappa) : fs;
    const float de = j > 0 ? fe - pm_flux<OPTION>(c - in[q - 1], kappa) : fe;
    out[q] = c + gamma * (ds + de);
  }
}

// ---- min / max ------------------------------------------------------------------------------------------------------
// part[2 b], part[2 b + 1] = min, max of workgroup b's share; the host finishes the few hundred partials
__global__ __launch_bounds__(256) void minmax_kernel(const double* __restrict__ img, int64_t n, double* __restrict__ part) {
  __shared__ double smn[4], smx[4];
  double mn = img[0], mx = img[0];
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
    const double v = img[q];
    mn = v < mn ? v : mn;
    mx = mx < v ? v : mx;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double a = __shfl_down(mn, off, 64), b = __shfl_down(mx, off, 64);
    mn = a < mn ? a : mn;
    mx = mx < b ? b : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = mn;
    smx[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      mn = smn[w] < mn ? smn[w] : mn;
      mx = mx < smx[w] ? smx[w] : mx;
    }
    part[2 * blockIdx.x] = mn;
    part[2 * blockIdx.x + 1] = mx;
  }
}

// ---- bilateral ------------------------------------------------------------------------------------------------------
constexpr int BL_TILE = 64;                   // output tile: 64 x 64
constexpr int BL_ROWS = 4;                    // consecutive rows of one column per thread
constexpr int BL_THREADS = BL_TILE * BL_TILE / BL_ROWS;
constexpr size_t LDS_BYTES = 160 * 1024;

// X consecutive taps of halo row y (window row t - k for the thread's output k) into the outputs K0 .. K1 it feeds.  The
// spatial weights (the same tap in every lane: scalar loads) and the halo values are fetched first, then the colour-table
// gathers of all the taps are in flight together; every output still adds its taps in ascending x
template <int K0, int K1, int X, class At>
__device__ __forceinline__ void bilateral_taps(At at, int y, int c, int t, int x, int win,
                                               const double* __restrict__ range_lut, const double* __restrict__ lut,
                                               double dist_scale, int bin_max, const double (&centre)[BL_ROWS],
                                               double (&total)[BL_ROWS], double (&weight_sum)[BL_ROWS]) {
  double rl[BL_ROWS][X], value[X], cw[BL_ROWS][X];
#pragma unroll
  for (int k = K0; k <= K1; ++k)
#pragma unroll
    for (int u = 0; u < X; ++u) rl[k][u] = range_lut[(t - k) * win + x + u];
#pragma unroll
  for (int u = 0; u < X; ++u) value[u] = at(y, c + x + u);
#pragma unroll
  for (int u = 0; u < X; ++u)
#pragma unroll
    for (int k = K0; k <= K1; ++k) {
      int bin = (int)(fabs(centre[k] - value[u]) * dist_scale);        // the host's (int64) truncation: >= 0, saturating
      bin = bin < bin_max ? bin : bin_max;
      cw[k][u] = lut[bin];
    }
#pragma unroll
  for (int u = 0; u < X; ++u)
#pragma unroll
    for (int k = K0; k <= K1; ++k) {
      const double w = rl[k][u] * cw[k][u];
      total[k] += value[u] * w;
      weight_sum[k] += w;
    }
}

template <int K0, int K1, class At>
__device__ __forceinline__ void bilateral_row(At at, int y, int c, int t, int win, const double* __restrict__ range_lut,
                                              const double* __restrict__ lut, double dist_scale, int bin_max,
                                              const double (&centre)[BL_ROWS], double (&total)[BL_ROWS],
                                              double (&weight_sum)[BL_ROWS]) {
  int x = 0;
  for (; x + 4 <= win; x += 4)
    bilateral_taps<K0, K1, 4>(at, y, c, t, x, win, range_lut, lut, dist_scale, bin_max, centre, total, weight_sum);
  for (; x < win; ++x)
    bilateral_taps<K0, K1, 1>(at, y, c, t, x, win, range_lut, lut, dist_scale, bin_max, centre, total, weight_sum);
}

template <bool TILE_LDS, bool LUT_LDS>
__global__ __launch_bounds__(BL_THREADS) void bilateral_kernel(const double* __restrict__ img, double* __restrict__ out, int H,
                                                               int W, int win, int bins, double dist_scale,
                                                               const double* __restrict__ range_lut,
                                                               const double* __restrict__ color_lut) {
  extern __shared__ double smem[];
  double* lut_s = smem;                                   // [bins] with LUT_LDS
  double* tile = smem + (LUT_LDS ? bins : 0);             // [(63 + win) x pitch] with TILE_LDS
  const int ext = (win - 1) / 2;
  const int pitch = BL_TILE + win - 1;
  const int64_t y0 = (int64_t)blockIdx.y * BL_TILE - ext, x0 = (int64_t)blockIdx.x * BL_TILE - ext;
  const int tid = threadIdx.x;
  if (LUT_LDS)
    for (int b = tid; b < bins; b += BL_THREADS) lut_s[b] = color_lut[b];
  if (TILE_LDS)
    for (int q = tid; q < pitch * pitch; q += BL_THREADS) {
      const int y = q / pitch, x = q - y * pitch;
      const int64_t gy = y0 + y, gx = x0 + x;
      tile[q] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? img[gy * W + gx] : 0.0;
    }
  __syncthreads();
  const double* lut = LUT_LDS ? lut_s : color_lut;
  auto at = [&](int y, int x) -> double {
    if (TILE_LDS) return tile[y * pitch + x];
    const int64_t gy = y0 + y, gx = x0 + x;
    return (gy >= 0 && gy < H && gx >= 0 && gx < W) ? img[gy * W + gx] : 0.0;
  };
  const int c = tid & (BL_TILE - 1), r0 = (tid / BL_TILE) * BL_ROWS;
  double centre[BL_ROWS], total[BL_ROWS], weight_sum[BL_ROWS];
#pragma unroll
  for (int k = 0; k < BL_ROWS; ++k) {
    centre[k] = at(r0 + k + ext, c + ext);
    total[k] = 0.0;
    weight_sum[k] = 0.0;
  }
  // halo row r0 + t is window row t - k of output k: outputs max(0, t - win + 1) .. min(3, t)
#define BL_CASE(K0, K1)                                                                                                   \
  case (K0) * BL_ROWS + (K1):                                                                                             \
    bilateral_row<K0, K1>(at, r0 + t, c, t, win, range_lut, lut, dist_scale, bins - 1, centre, total, weight_sum);        \
    break;
  for (int t = 0; t < win + BL_ROWS - 1; ++t) {
    const int klo = t - (win - 1) > 0 ? t - (win - 1) : 0, khi = t < BL_ROWS - 1 ? t : BL_ROWS - 1;
    switch (klo * BL_ROWS + khi) {
      BL_CASE(0, 0) BL_CASE(0, 1) BL_CASE(0, 2) BL_CASE(0, 3) BL_CASE(1, 1) BL_CASE(1, 2) BL_CASE(1, 3) BL_CASE(2, 2)
      BL_CASE(2, 3) BL_CASE(3, 3)
    }
  }
#undef BL_CASE
  const int64_t gx = (int64_t)blockIdx.x * BL_TILE + c;
#pragma unroll
  for (int k = 0; k < BL_ROWS; ++k) {
    const int64_t gy = (int64_t)blockIdx.y * BL_TILE + r0 + k;
    if (gy < H && gx < W) out[gy * W + gx] = total[k] / weight_sum[k];
  }
}

template <bool TILE_LDS, bool LUT_LDS>
int launch_bilateral(const double* img, double* out, int H, int W, int win, int bins, double dist_scale,
                     const double* range_lut, const double* color_lut, size_t lds, hipStream_t st) {
  auto* fn = bilateral_kernel<TILE_LDS, LUT_LDS>;
  if (lds > 64 * 1024)
    PHMRF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(fn, dim3((W + BL_TILE - 1) / BL_TILE, (H + BL_TILE - 1) / BL_TILE), dim3(BL_THREADS), lds, st, img, out,
                     H, W, win, bins, dist_scale, range_lut, color_lut);
  PHMRF_HIP(hipGetLastError());
  return PHMRF_OK;
}

// ---- gaussian -------------------------------------------------------------------------------------------------------
// scipy's `reflect`: d c b a | a b c d | d c b a, with period 2 n however far the index lies outside
__device__ __forceinline__ int reflect_index(int64_t i, int n) {
  const int64_t p = 2 * (int64_t)n;
  int64_t m = i % p;
  if (m < 0) m += p;
  return (int)(m >= n ? p - 1 - m : m);
}

// one axis of scipy's correlate1d with a symmetric kernel: centre first, then the pairs from the farthest inwards
template <int AXIS>
__global__ __launch_bounds__(256) void gaussian_pass_kernel(const double* __restrict__ in, double* __restrict__ out, int H,
                                                            int W, int radius, const double* __restrict__ weights) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= W) return;
  const int n = AXIS == 0 ? H : W;
  for (int i = blockIdx.y * ROWS_PER_WG + threadIdx.y; i < H; i += gridDim.y * ROWS_PER_WG) {
    const int at = AXIS == 0 ? i : j;
    const int64_t line = AXIS == 0 ? (int64_t)j : (int64_t)i * W, step = AXIS == 0 ? (int64_t)W : 1;
    double acc = in[line + at * step] * weights[radius];
    const bool inside = at - radius >= 0 && at + radius < n;
    for (int d = radius; d >= 1; --d) {
      const int lo = inside ? at - d : reflect_index((int64_t)at - d, n);
      const int hi = inside ? at + d : reflect_index((int64_t)at + d, n);
      acc += (in[line + lo * step] + in[line + hi * step]) * weights[radius - d];
    }
    out[(int64_t)i * W + j] = acc;
  }
}

int check_plane(const void* a, const void* b, int64_t H, int64_t W) {
  PHMRF_CHECK(a && b, PHMRF_ERR_INVALID, "NULL image buffer");
  PHMRF_CHECK(H >= 1 && W >= 1, PHMRF_ERR_INVALID, "H and W must be >= 1");
  PHMRF_CHECK(H < ((int64_t)1 << 31) && W < ((int64_t)1 << 31) && H * W < ((int64_t)1 << 31) - 64, PHMRF_ERR_UNSUPPORTED,
              "the plane must have fewer than 2^31 - 64 pixels");
  return PHMRF_OK;
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_filter_diffusion(float* img_dev, float* tmp_dev, int64_t H, int64_t W, int niter, double kappa, double gamma,
                           int option, void* hip_stream) {
  PHMRF_TRY(check_plane(img_dev, tmp_dev, H, W));
  PHMRF_CHECK(niter >= 0, PHMRF_ERR_INVALID, "niter must be >= 0");
  PHMRF_CHECK(option == 1 || option == 2, PHMRF_ERR_INVALID, "option must be 1 or 2");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const dim3 grid = plane_grid(H, W), tb(64, ROWS_PER_WG);
  float* src = img_dev;
  float* dst = tmp_dev;
  for (int it = 0; it < niter; ++it) {
    if (option == 1)
      hipLaunchKernelGGL(diffusion_step_kernel<1>, grid, tb, 0, st, src, dst, (int)H, (int)W, (float)kappa, (float)gamma);
    else
      hipLaunchKernelGGL(diffusion_step_kernel<2>, grid, tb, 0, st, src, dst, (int)H, (int)W, (float)kappa, (float)gamma);
    std::swap(src, dst);
  }
  PHMRF_HIP(hipGetLastError());
  if (src != img_dev)
    PHMRF_HIP(hipMemcpyAsync(img_dev, src, (size_t)(H * W) * sizeof(float), hipMemcpyDeviceToDevice, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  return PHMRF_OK;
}

int phmrf_filter_bilateral(const double* img_dev, double* out_dev, int64_t H, int64_t W, double sigma_color,
                           double sigma_spatial, int win_size, int bins, void* hip_stream) {
  PHMRF_TRY(check_plane(img_dev, out_dev, H, W));
  PHMRF_CHECK(sigma_color > 0.0 && sigma_spatial > 0.0, PHMRF_ERR_INVALID, "the sigmas must be positive");
  if (bins <= 0) bins = 10000;
  if (win_size <= 0) win_size = std::max(5, 2 * (int)std::ceil(3.0 * sigma_spatial) + 1);
  PHMRF_CHECK(win_size % 2 == 1, PHMRF_ERR_INVALID, "the window must be odd");
  PHMRF_CHECK(win_size <= 4095, PHMRF_ERR_UNSUPPORTED, "the window must be <= 4095");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int64_t n = H * W;

  Buffers buf;
  double *lut_a, *lut_b;             // a: min / max partials, then the colour table; b: the spatial table
  const int g = (int)std::min<int64_t>(1024, (n + 255) / 256);
  PHMRF_TRY(buf.get(&lut_a, std::max<size_t>((size_t)2 * g, (size_t)bins)));
  hipLaunchKernelGGL(minmax_kernel, dim3(g), dim3(256), 0, st, img_dev, n, lut_a);
  PHMRF_HIP(hipGetLastError());
  std::vector<double> part((size_t)2 * g);
  PHMRF_HIP(hipMemcpyAsync(part.data(), lut_a, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  double mn = part[0], mx = part[1];
  for (int b = 1; b < g; ++b) {
    mn = std::min(mn, part[2 * b]);
    mx = std::max(mx, part[2 * b + 1]);
  }
  if (mn == mx) {
    if (img_dev != out_dev) PHMRF_HIP(hipMemcpyAsync(out_dev, img_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    PHMRF_HIP(hipStreamSynchronize(st));
    return PHMRF_OK;
  }
  PHMRF_CHECK(!(mn < 0.0) && mx != 0.0, PHMRF_ERR_INVALID, "the image must hold no negative value");
  PHMRF_CHECK(img_dev != out_dev, PHMRF_ERR_INVALID, "the bilateral filter does not run in place");

  // both tables with the expressions of preprocess_host.cpp, so that the two libraries hold the same numbers
  const int ext = (win_size - 1) / 2;
  std::vector<double> color_lut((size_t)bins), range_lut((size_t)win_size * win_size);
  for (int b = 0; b < bins; ++b) {
    const double v = (double)b * mx / (double)bins / sigma_color;
    color_lut[(size_t)b] = std::exp(-0.5 * v * v);
  }
  for (int kr = 0; kr < win_size; ++kr)
    for (int kc = 0; kc < win_size; ++kc) {
      const double d = std::sqrt((double)((kr - ext) * (kr - ext) + (kc - ext) * (kc - ext))) / sigma_spatial;
      range_lut[(size_t)kr * win_size + kc] = std::exp(-0.5 * d * d);
    }
  const double dist_scale = (double)bins / mx;
  PHMRF_TRY(buf.get(&lut_b, range_lut.size()));
  PHMRF_HIP(hipMemcpyAsync(lut_a, color_lut.data(), color_lut.size() * sizeof(double), hipMemcpyHostToDevice, st));
  PHMRF_HIP(hipMemcpyAsync(lut_b, range_lut.data(), range_lut.size() * sizeof(double), hipMemcpyHostToDevice, st));

  // LDS: the tile first, the colour table beside it when both fit
  const size_t pitch = (size_t)BL_TILE + win_size - 1;
  const size_t tile_bytes = pitch * pitch * sizeof(double), lut_bytes = (size_t)bins * sizeof(double);
  const bool tile_lds = tile_bytes <= LDS_BYTES;
#ifdef PHMRF_BILATERAL_LUT_GLOBAL            // A/B build of the colour table's placement
  const bool lut_lds = false;
#else
  const bool lut_lds = (tile_lds ? tile_bytes : 0) + lut_bytes <= LDS_BYTES;
#endif
  const size_t lds = (tile_lds ? tile_bytes : 0) + (lut_lds ? lut_bytes : 0);
  if (tile_lds && lut_lds)
    PHMRF_TRY((launch_bilateral<true, true>(img_dev, out_dev, (int)H, (int)W, win_size, bins, dist_scale, lut_b, lut_a, lds, st)));
  else if (tile_lds)
    PHMRF_TRY((launch_bilateral<true, false>(img_dev, out_dev, (int)H, (int)W, win_size, bins, dist_scale, lut_b, lut_a, lds, st)));
  else if (lut_lds)
    PHMRF_TRY((launch_bilateral<false, true>(img_dev, out_dev, (int)H, (int)W, win_size, bins, dist_scale, lut_b, lut_a, lds, st)));
  else
    PHMRF_TRY((launch_bilateral<false, false>(img_dev, out_dev, (int)H, (int)W, win_size, bins, dist_scale, lut_b, lut_a, lds, st)));
  PHMRF_HIP(hipStreamSynchronize(st));
  return PHMRF_OK;
}

int phmrf_filter_gaussian(const double* img_dev, double* out_dev, double* tmp_dev, int64_t H, int64_t W, double sigma,
                          double truncate, void* hip_stream) {
  PHMRF_TRY(check_plane(img_dev, out_dev, H, W));
  PHMRF_CHECK(tmp_dev, PHMRF_ERR_INVALID, "NULL scratch buffer");
  PHMRF_CHECK(sigma > 0.0 && truncate > 0.0, PHMRF_ERR_INVALID, "sigma and truncate must be positive");
  PHMRF_CHECK(img_dev != out_dev && img_dev != tmp_dev && tmp_dev != out_dev, PHMRF_ERR_INVALID,
              "image, output and scratch must be three buffers");
  PHMRF_CHECK(truncate * sigma + 0.5 < 1e6, PHMRF_ERR_UNSUPPORTED, "the radius must be below 10^6");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int radius = (int)(truncate * sigma + 0.5);
  // scipy's _gaussian_kernel1d: exp(-0.5 / sigma^2 * x^2), normalised
  std::vector<double> weights((size_t)2 * radius + 1);
  const double sigma2 = sigma * sigma;
  double sum = 0.0;
  for (int x = -radius; x <= radius; ++x) {
    weights[(size_t)(x + radius)] = std::exp(-0.5 / sigma2 * (double)(x * (int64_t)x));
    sum += weights[(size_t)(x + radius)];
  }
  for (double& v : weights) v /= sum;
  Buffers buf;
  double* weights_dev;
  PHMRF_TRY(buf.get(&weights_dev, weights.size()));
  PHMRF_HIP(hipMemcpyAsync(weights_dev, weights.data(), weights.size() * sizeof(double), hipMemcpyHostToDevice, st));
  const dim3 grid = plane_grid(H, W), tb(64, ROWS_PER_WG);
  hipLaunchKernelGGL(gaussian_pass_kernel<0>, grid, tb, 0, st, img_dev, tmp_dev, (int)H, (int)W, radius, weights_dev);
  hipLaunchKernelGGL(gaussian_pass_kernel<1>, grid, tb, 0, st, tmp_dev, out_dev, (int)H, (int)W, radius, weights_dev);
  PHMRF_HIP(hipGetLastError());
  PHMRF_HIP(hipStreamSynchronize(st));
  return PHMRF_OK;
}

}  // extern "C"
