// gfx950 kernels that draw ONE state map of one region as an image (phmrf_render_states).  Integer
// arithmetic throughout: no result depends on the order in which the atomics land.
//
//   vote     the region's full matrix M (a diagonal block: M[i][j] = the stored node (min(i, j), max(i, j))) is reduced by an
//            integer factor f: pixel (p, q) covers the cells [p f, (p + 1) f) x [q f, (q + 1) f) cut at H and W.  A workgroup
//            owns a TILE of RENDER_TILE consecutive pixels of one pixel row, the tiles stride over a capped grid.  Its lanes
//            walk the tile's source cells along the storage rows (coalesced loads) and count per (pixel, state) in u32 bins
//            in LDS, ONE LDS atomic per run of equal (pixel, state) among consecutive lanes (wave_run_add).  Eight lanes per
//            pixel then take the state with the largest count (the lowest on ties) and leave the bins zeroed.  With
//            confidences a SECOND sweep over the same cells adds floor(conf 2^24) of the winner's cells into one u64 per
//            pixel (and checks every confidence it passes); the tile's pixels are then written.
//            A diagonal block's image is symmetric (the pixel grid is the same on both axes): only the pixels p <= q are
//            voted, from the stored cells alone, and written at (p, q) and (q, p).  A pixel p == q holds the cells i <= j of
//            its square: those with i < j count twice, as on the full matrix.  The tiles of a diagonal block are the upper
//            triangle of the tile grid, 32 pixel rows per tile of that triangle.
//            The kernel visits every stored node exactly once, so it is also the input check: a label >= K, a confidence
//            that is not a finite number in [0, 1].
//   colour   per pixel from the three planes: highlight for a marked pixel, the outline colour where the state differs
//            from the pixel to the right or below, else the state's palette colour faded towards white by 1 - conf8 / 255.

#include "runs.h"

namespace phmrf {
namespace {

constexpr int RENDER_GRID_CAP = 1024;    // workgroups of both kernels (render.py GRID_CAP)
constexpr int RENDER_TILE = 32;          // pixels of a tile (render.py TILE)
constexpr int RENDER_STRIDE = 65;        // u32 bins per pixel: 64 states and one word that keeps the pixels' rows off one bank
constexpr int RENDER_MAX_FACTOR = 32768; // a pixel's count stays below 2^31: f^2 cells, the mirrored ones twice

// the source cells of one tile: rows [i0, i0 + nr), columns [j0, j0 + nc) of the full matrix; pixels q0 .. q0 + npix - 1 of
// pixel row p (a diagonal block: q0 >= p)
struct RenderTile {
  int p, q0, npix, i0, nr, j0, nc;
};

// tile T of the region; false for a tile of the last rows' padding (a diagonal block: pixel rows h .. 32 ceil(h / 32) - 1)
__device__ __forceinline__ bool render_tile(int64_t T, int H, int W, int h, int w, int diagonal, int f, int per_row,
                                            RenderTile* t) {
  int p, tq;
  if (diagonal) {                                      // the upper triangle of the per_row x per_row tile grid, 32 rows each
    int g;
    grid_coords(T >> 5, per_row, 1, &g, &tq);
    p = g * RENDER_TILE + (int)(T & 31);
  } else {
    grid_coords(T, per_row, 0, &p, &tq);
  }
  if (p >= h) return false;
  int64_t q0 = (int64_t)tq * RENDER_TILE, q1 = q0 + RENDER_TILE;
  if (diagonal && q0 < p) q0 = p;
  if (q1 > w) q1 = w;
  const int64_t i1 = ((int64_t)p + 1) * f < H ? ((int64_t)p + 1) * f : H;
  const int64_t j1 = q1 * f < W ? q1 * f : W;
  t->p = p;
  t->q0 = (int)q0;
  t->npix = (int)(q1 - q0);
  t->i0 = p * f;
  t->nr = (int)(i1 - t->i0);
  t->j0 = (int)(q0 * f);
  t->nc = (int)(j1 - t->j0);
  return true;
}

// body(v, px, weight) for every lane and trip, the same number of trips for all 256 lanes: v the stored node of the lane's
// cell or -1 (past the tile's end, or below the diagonal), px the cell's pixel within the tile, weight 2 for a cell that
// stands for its mirror image too.  Consecutive lanes take consecutive cells of a storage row.
template <class F>
__device__ __forceinline__ void render_walk(const RenderTile& t, int f, int W, int diagonal, F&& body) {
  const int64_t total = (int64_t)t.nr * t.nc;
  int r = (int)threadIdx.x / t.nc, c = (int)threadIdx.x % t.nc;
  for (int64_t base = 0; base < total; base += 256) {
    int64_t v = -1;
    int px = 0, weight = 0;
    if (base + threadIdx.x < total) {
      const int i = t.i0 + r, j = t.j0 + c;
      if (!diagonal || i <= j) {
        v = grid_id<int64_t>(i, j, W, diagonal);
        px = c / f;
        weight = (diagonal && i < j && t.q0 + px == t.p) ? 2 : 1;
      }
    }
    body(v, px, weight);
    c += 256;
    if (c >= t.nc) {
      const int k = c / t.nc;
      r += k;
      c -= k * t.nc;
    }
  }
}

// planes: [3][h w] state, conf8, mark8.  bad |= 1 for a label >= K, 2 for a confidence that is not a finite number in [0, 1]
__global__ __launch_bounds__(256) void render_vote_kernel(const uint8_t* __restrict__ labels, const float* __restrict__ conf,
                                                          const uint8_t* __restrict__ mark, int H, int W, int diagonal, int K,
                                                          int f, int h, int w, int per_row, int64_t ntiles,
                                                          uint8_t* __restrict__ planes, int* __restrict__ bad) {
  __shared__ unsigned bins[RENDER_TILE * RENDER_STRIDE];
  __shared__ unsigned long long sums[RENDER_TILE];
  __shared__ unsigned count_of[RENDER_TILE];
  __shared__ int winner[RENDER_TILE];
  __shared__ unsigned marked[RENDER_TILE];
  for (int t = threadIdx.x; t < RENDER_TILE * RENDER_STRIDE; t += 256) bins[t] = 0;
  if (threadIdx.x < RENDER_TILE) {
    sums[threadIdx.x] = 0;
    marked[threadIdx.x] = 0;
  }
  __syncthreads();
  const int64_t plane = (int64_t)h * w;
  int wrong = 0;
  for (int64_t T = blockIdx.x; T < ntiles; T += gridDim.x) {
    RenderTile t;
    if (!render_tile(T, H, W, h, w, diagonal, f, per_row, &t)) continue;        // (the same for the whole workgroup)
    render_walk(t, f, W, diagonal, [&](int64_t v, int px, int weight) {
      int key = -1;
      if (v >= 0) {
        const int s = labels[v];
        if (s >= K) wrong |= 1;
        else key = px * RENDER_STRIDE + s;
        if (mark && mark[v]) marked[px] = 1;
      }
      wave_run_add(bins, key, key >= 0 ? (unsigned)weight : 0u);
    });
    __syncthreads();
    {                                                  // eight lanes per pixel: the largest count, the lowest state on ties
      const int px = threadIdx.x >> 3, part = threadIdx.x & 7;
      unsigned long long best = 0;
      for (int k = part; k < K; k += 8) {
        const unsigned long long cand = ((unsigned long long)bins[px * RENDER_STRIDE + k] << 6) | (unsigned)(63 - k);
        bins[px * RENDER_STRIDE + k] = 0;
        best = cand > best ? cand : best;
      }
#pragma unroll
      for (int off = 4; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(best, off, 64);
        best = other > best ? other : best;
      }
      if (part == 0) {
        winner[px] = 63 - (int)(best & 63ull);
        count_of[px] = (unsigned)(best >> 6);
      }
    }
    __syncthreads();
    if (conf) {
      render_walk(t, f, W, diagonal, [&](int64_t v, int px, int weight) {
        int key = -1;
        unsigned long long x = 0;
        if (v >= 0) {
          const float c = conf[v];
          if (!unit_conf(c)) wrong |= 2;
          else if ((int)labels[v] == winner[px]) {
            key = px;
            x = (unsigned long long)weight * (unsigned long long)(c * 16777216.0f);   // exact: a float32 in [0, 1] times 2^24
          }
        }
        wave_run_add(sums, key, x);
      });
      __syncthreads();
    }
    if ((int)threadIdx.x < RENDER_TILE) {
      const int px = threadIdx.x;
      if (px < t.npix) {
        const unsigned cells = count_of[px];
        const uint8_t state = (uint8_t)winner[px];
        const uint8_t conf8 = (conf && cells) ? (uint8_t)((255ull * sums[px]) / ((unsigned long long)cells << 24)) : 255;
        const uint8_t mark8 = marked[px] ? 1 : 0;
        const int q = t.q0 + px;
        const int64_t at = (int64_t)t.p * w + q, mirror = (int64_t)q * w + t.p;
        planes[at] = state;
        planes[plane + at] = conf8;
        planes[2 * plane + at] = mark8;
        if (diagonal) {
          planes[mirror] = state;
          planes[plane + mirror] = conf8;
          planes[2 * plane + mirror] = mark8;
        }
      }
      sums[px] = 0;
      marked[px] = 0;
    }
    __syncthreads();
  }
  if (wrong) atomicOr(bad, wrong);
}

// colours: [K][3] palette, then the highlight and the outline colour
__global__ __launch_bounds__(256) void render_colour_kernel(const uint8_t* __restrict__ planes, int h, int w, int K, int outline,
                                                            const uint8_t* __restrict__ colours, uint8_t* __restrict__ rgb) {
  const int64_t plane = (int64_t)h * w;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < plane; x += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(x / w), q = (int)(x - (int64_t)p * w);
    const int s = planes[x];
    const uint8_t* from;
    int t = 255;
    if (planes[2 * plane + x]) {
      from = colours + 3 * K;
    } else if (outline && ((q + 1 < w && planes[x + 1] != s) || (p + 1 < h && planes[x + w] != s))) {
      from = colours + 3 * K + 3;
    } else {
      from = colours + 3 * s;
      t = 64 + (191 * (int)planes[plane + x]) / 255;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[3 * x + c] = (uint8_t)(255 - ((255 - (int)from[c]) * t) / 255);
  }
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_render_states(const uint8_t* labels_dev, const float* conf_dev_or_null, const uint8_t* mark_dev_or_null, int H, int W,
                        int diagonal, int K, int factor, const uint8_t* palette_host, const uint8_t* extra_host, int outline,
                        uint8_t* planes_host_or_null, uint8_t* rgb_host_or_null, void* hip_stream) {
  PHMRF_CHECK(labels_dev && palette_host && extra_host, PHMRF_ERR_INVALID, "NULL labels, palette or extra colours");
  PHMRF_TRY(check_region(H, W, diagonal));
  PHMRF_CHECK(K >= 1 && K <= 64, PHMRF_ERR_INVALID, "K must be in 1 .. 64");
  PHMRF_CHECK(factor >= 1, PHMRF_ERR_INVALID, "factor must be >= 1");
  PHMRF_CHECK(factor <= RENDER_MAX_FACTOR, PHMRF_ERR_UNSUPPORTED, "factor must be <= 32768");
  const int64_t h = ((int64_t)H + factor - 1) / factor, w = ((int64_t)W + factor - 1) / factor;
  PHMRF_CHECK(h * w < ((int64_t)1 << 31) - 64, PHMRF_ERR_UNSUPPORTED, "the image must have fewer than 2^31 - 64 pixels");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const size_t plane = (size_t)(h * w);
  const int per_row = (int)((w + RENDER_TILE - 1) / RENDER_TILE);
  const int64_t ntiles = diagonal ? (int64_t)RENDER_TILE * grid_row_first<int64_t>(per_row, per_row, 1) : h * per_row;

  Buffers buf;
  uint8_t* planes;
  int* flag;
  PHMRF_TRY(buf.get(&planes, 3 * plane));
  PHMRF_TRY(buf.get(&flag, 1));
  PHMRF_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  hipLaunchKernelGGL(render_vote_kernel, dim3(grid_of(ntiles, 1, RENDER_GRID_CAP)), dim3(256), 0, st, labels_dev, conf_dev_or_null,
                     mark_dev_or_null, H, W, diagonal, K, factor, (int)h, (int)w, per_row, ntiles, planes, flag);
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  PHMRF_CHECK(!(bad & 1), PHMRF_ERR_INVALID, "a label is >= K");
  PHMRF_CHECK(!(bad & 2), PHMRF_ERR_INVALID, "a confidence is not a finite number in [0, 1]");
  if (rgb_host_or_null) {
    std::vector<uint8_t> colours((size_t)3 * K + 6);
    for (int t = 0; t < 3 * K; ++t) colours[(size_t)t] = palette_host[t];
    for (int t = 0; t < 6; ++t) colours[(size_t)3 * K + t] = extra_host[t];
    uint8_t *rgb, *colours_dev;
    PHMRF_TRY(buf.get(&rgb, 3 * plane));
    PHMRF_TRY(buf.get(&colours_dev, colours.size()));
    PHMRF_HIP(hipMemcpyAsync(colours_dev, colours.data(), colours.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(render_colour_kernel, dim3(grid_of((int64_t)plane, 256, RENDER_GRID_CAP)), dim3(256), 0, st, planes,
                       (int)h, (int)w, K, outline ? 1 : 0, colours_dev, rgb);
    PHMRF_HIP(hipGetLastError());
    PHMRF_HIP(hipMemcpyAsync(rgb_host_or_null, rgb, 3 * plane, hipMemcpyDeviceToHost, st));
  }
  if (planes_host_or_null)
    PHMRF_HIP(hipMemcpyAsync(planes_host_or_null, planes, 3 * plane, hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  return PHMRF_OK;
}

}  // extern "C"
