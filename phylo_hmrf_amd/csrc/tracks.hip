// gfx950 kernel that projects ONE state map of one region onto its two genome axes (phmrf_state_tracks).
// Integer arithmetic throughout: no result depends on the order in which the atomics land.
//
//   count    rows[i][k] / cols[j][k]: the cells of row i / column j of the region's full matrix M (a diagonal block:
//            M[i][j] = the stored node (min(i, j), max(i, j))) that hold state k and lie INSIDE the distance window
//            d_lo <= |dist0 + j - i| <= d_hi.  A workgroup owns a TILE of TRACKS_TILE_H storage rows by TRACKS_TILE_W storage
//            columns, the tiles stride over a capped grid.  A tile wholly outside the window is left without a load, a tile
//            wholly inside it drops the per-cell test.  A wave takes every fourth storage row of the tile, one at a time, and
//            issues the loads of all its rows before it counts the first.  Per row: up to three head bytes to the next
//            4-byte boundary of the row's address, then one 4-byte load per lane (four labels), then up to three tail bytes;
//            the head and tail go byte-wise on the first lanes.  So the lanes of a wave hold distinct columns of ONE row.
//            Two u32 tables in LDS, (tile row, state) and (tile column, state), both with a row stride of TRACKS_STRIDE = 65
//            words.  The row table takes ONE atomic per run of equal state among consecutive lanes (wave_run_add; what is
//            left of a lane's four after a change of state goes in singly).  The column table takes one atomic per cell;
//            only other waves can hit the same word.  The lanes take their four columns in a rotated order (lane >> 3), so
//            that 32 lanes of equal state fall on 32 banks instead of 8.
//            The flush adds every non-zero word of the two tables to the device table with one global atomic and zeroes it.
//            A diagonal block has one device table: a stored node (i, j) with i < j counts for bin i (row table) and for bin
//            j (column table, flushed into the same rows), a node of the diagonal for bin i alone.  Its tiles are the upper
//            triangle of the grid of TRACKS_TILE_W-square super-tiles, TRACKS_TILE_W / TRACKS_TILE_H tiles each.
//            A label >= K inside the window sets a flag; nodes outside the window are not inspected.

#include "runs.h"

namespace phmrf {
namespace {

constexpr int TRACKS_GRID_CAP = 1024;    // workgroups of the kernel (tracks.py GRID_CAP)
constexpr int TRACKS_TILE_H = 32;        // storage rows of a tile (tracks.py TILE_H)
constexpr int TRACKS_TILE_W = 256;       // storage columns of a tile: 64 lanes x 4 labels (tracks.py TILE_W)
constexpr int TRACKS_STRIDE = 65;        // u32 words per tile row / column: 64 states and one word that keeps neighbours off one bank
constexpr int TRACKS_ROWS_PER_WAVE = TRACKS_TILE_H / 4;          // a workgroup is four waves

// table: u32 [(H + W) K], the rows' counts and then the columns' (a diagonal block: [H K]); d_hi: INT_MAX for no upper limit
__global__ __launch_bounds__(256) void tracks_kernel(const uint8_t* __restrict__ labels, int H, int W, int diagonal, int dist0,
                                                     int K, int d_lo, int d_hi, int per_row, int64_t ntiles,
                                                     unsigned* __restrict__ table, int* __restrict__ bad) {
  __shared__ unsigned row_tab[TRACKS_TILE_H * TRACKS_STRIDE];
  __shared__ unsigned col_tab[TRACKS_TILE_W * TRACKS_STRIDE];
  for (int t = threadIdx.x; t < TRACKS_TILE_H * TRACKS_STRIDE; t += 256) row_tab[t] = 0;
  for (int t = threadIdx.x; t < TRACKS_TILE_W * TRACKS_STRIDE; t += 256) col_tab[t] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rot = (lane >> 3) & 3;
  unsigned* const col_out = table + (diagonal ? (size_t)0 : (size_t)H * K);
  bool wrong = false;
  for (int64_t T = blockIdx.x; T < ntiles; T += gridDim.x) {
    WindowTile t;
    if (!window_tile<TRACKS_TILE_H, TRACKS_TILE_W>(T, H, W, diagonal, per_row, dist0, d_lo, d_hi, &t)) continue;
    uint32_t word[TRACKS_ROWS_PER_WAVE];
    int single[TRACKS_ROWS_PER_WAVE];
    load_tile_rows<4>(labels, t, W, diagonal, wave, lane, word, single);    // the wave's rows i0 + wave, i0 + wave + 4, ...
#pragma unroll
    for (int u = 0; u < TRACKS_ROWS_PER_WAVE; ++u) {
      const int i = t.i0 + wave + 4 * u;
      if (i >= t.i1) break;
      const LabelRow r = label_row(labels, i, t.j0, t.j1, W, diagonal);
      const int row_key = (i - t.i0) * TRACKS_STRIDE;
      const int x0 = dist0 - i;                                         // the cell's distance is |x0 + j|
      // one cell: -1 outside the window or with a label >= K, else the state; the column table takes it here
      auto cell = [&](int s, int j) -> int {
        if (!t.whole) {
          const int x = x0 + j, d = x < 0 ? -x : x;
          if (d < d_lo || d > d_hi) return -1;
        }
        if (s >= K) {
          wrong = true;
          return -1;
        }
        if (!diagonal || j != i) atomicAdd(col_tab + (j - t.j0) * TRACKS_STRIDE + s, 1u);
        return s;
      };
      if (r.nvec > 0) {
        int key[4] = {-1, -1, -1, -1};
        if (lane < r.nvec) {
          const uint32_t w = __builtin_rotateright32(word[u], 8 * rot);
          const int j = r.ja + r.head + 4 * lane;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int s = cell((int)((w >> (8 * e)) & 0xff), j + ((e + rot) & 3));
            key[e] = s < 0 ? -1 : row_key + s;
          }
        }
        wave_quad_add(row_tab, key);
      }
      if (r.nbytes > 0) {
        int key = -1;
        if (lane < r.nbytes) {
          const int s = cell(single[u], r.ja + r.byte_at(lane));
          key = s < 0 ? -1 : row_key + s;
        }
        wave_run_add(row_tab, key, key >= 0 ? 1u : 0u);
      }
    }
    __syncthreads();
    const int nr = t.i1 - t.i0, ncol = t.j1 - t.j0;
    for (int x = threadIdx.x; x < nr * K; x += 256) {
      const int r = x / K, s = x - r * K;
      const unsigned c = row_tab[r * TRACKS_STRIDE + s];
      if (c) {
        atomicAdd(table + (size_t)(t.i0 + r) * K + s, c);
        row_tab[r * TRACKS_STRIDE + s] = 0;
      }
    }
    for (int x = threadIdx.x; x < ncol * K; x += 256) {
      const int r = x / K, s = x - r * K;
      const unsigned c = col_tab[r * TRACKS_STRIDE + s];
      if (c) {
        atomicAdd(col_out + (size_t)(t.j0 + r) * K + s, c);
        col_tab[r * TRACKS_STRIDE + s] = 0;
      }
    }
    __syncthreads();
  }
  if (wrong) atomicOr(bad, 1);
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_state_tracks(const uint8_t* labels_dev, int H, int W, int diagonal, int64_t dist0, int K, int64_t d_min, int64_t d_max,
                       int64_t* rows_host, int64_t* cols_host_or_null, void* hip_stream) {
  PHMRF_CHECK(labels_dev && rows_host, PHMRF_ERR_INVALID, "NULL labels or rows");
  int64_t n;
  PHMRF_TRY(check_region(H, W, diagonal, &n));
  PHMRF_CHECK(diagonal || cols_host_or_null, PHMRF_ERR_INVALID, "an off-diagonal block needs cols");
  PHMRF_CHECK(!diagonal || dist0 == 0, PHMRF_ERR_INVALID, "a diagonal block has dist0 == 0");
  PHMRF_TRY(check_window(d_min, d_max));
  PHMRF_TRY(check_states(K));
  PHMRF_TRY(check_nodes(n, "n must be below 2^31 - 64"));
  PHMRF_TRY(check_span(dist0, H, W));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const size_t words = ((size_t)H + (diagonal ? 0 : (size_t)W)) * (size_t)K;
  int per_row;
  const int64_t ntiles = window_tile_count<TRACKS_TILE_H, TRACKS_TILE_W>(H, W, diagonal, &per_row);

  Buffers buf;
  unsigned* table;
  int* flag;
  PHMRF_TRY(buf.get(&table, words));
  PHMRF_TRY(buf.get(&flag, 1));
  PHMRF_HIP(hipMemsetAsync(table, 0, words * sizeof(unsigned), st));
  PHMRF_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  const IntWindow win = int_window(d_min, d_max);
  hipLaunchKernelGGL(tracks_kernel, dim3(grid_of(ntiles, 1, TRACKS_GRID_CAP)), dim3(256), 0, st, labels_dev, H, W, diagonal,
                     (int)dist0, K, win.lo, win.hi, per_row, ntiles, table, flag);
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  PHMRF_CHECK(!bad, PHMRF_ERR_INVALID, "a label inside the window is >= K");
  std::vector<unsigned> got(words);
  PHMRF_HIP(hipMemcpyAsync(got.data(), table, words * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  PHMRF_HIP(hipStreamSynchronize(st));
  const size_t nrow = (size_t)H * (size_t)K;
  for (size_t t = 0; t < nrow; ++t) rows_host[t] = (int64_t)got[t];
  if (!diagonal)
    for (size_t t = nrow; t < words; ++t) cols_host_or_null[t - nrow] = (int64_t)got[t];
  return PHMRF_OK;
}

}  // extern "C"
