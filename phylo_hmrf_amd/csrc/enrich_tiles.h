// What enrich.hip and enrich_null.hip share: the tile of the label kernels and the row a half-wave counts,
// the category of a bin pair, the class kernels' walk along the signed diagonals inside the distance window and the host's choice
// of those diagonals.  Where a bin's class and segment come from, and what a cell or a chunk is added to, is each kernel's own.
#pragma once

#include "runs.h"

namespace phmrf {

constexpr int ENRICH_TILE_H = 32;        // storage rows of a tile (enrich.py TILE_H)
constexpr int ENRICH_TILE_W = 128;       // storage columns of a tile: 32 lanes x 4 labels (enrich.py TILE_W)
constexpr int ENRICH_TILE_D = ENRICH_TILE_H + ENRICH_TILE_W - 1;   // distances of a tile
constexpr int ENRICH_PAIRS_PER_WAVE = ENRICH_TILE_H / 8;           // a workgroup is four waves of two rows each
constexpr int ENRICH_MAX_CLASSES = 8;
constexpr int ENRICH_MAX_PAIRS = 2 * ENRICH_MAX_CLASSES * ENRICH_MAX_CLASSES;
constexpr int BAD_LABEL = 1, BAD_CLASS = 2;                        // bits of the flag word

// row i of tile t as a half-wave counts it; the second row of a wave may be absent: then it holds no word and no byte
__device__ __forceinline__ LabelRow present_row(const uint8_t* __restrict__ labels, const WindowTile& t, int i, bool present, int W,
                                                int diagonal) {
  LabelRow r = label_row(labels, present ? i : t.i0, t.j0, t.j1, W, diagonal);
  if (!present) r.nvec = r.nbytes = 0;
  return r;
}

// the category of a bin pair from the (class < C, segment) of its row and column bin: `same` is one segment >= 0 on both sides
__device__ __forceinline__ int pair_bin(int2 mine, int2 other, int C) {
  const int same = (mine.y >= 0 && mine.y == other.y) ? 1 : 0;
  return (mine.x * C + other.x) * 2 + same;
}

// Item `item` of the walk along the signed diagonals x = dist0 + j - i inside the window: x = xa + t for t < na, x = xb +
// (t - na) for the diagonals after them; `slots` chunks of CHUNK rows cover the longest diagonal; item = t slots + slot.  Gives
// x, shift = j - i and the rows [a, b) of the chunk; false for a slot past the diagonal's end (the same for the wave).
template <int CHUNK>
__device__ __forceinline__ bool diagonal_chunk(int64_t item, int slots, int xa, int na, int xb, int dist0, int H, int W, int* x,
                                               int* shift, int* a, int* b) {
  const int t = (int)(item / slots), slot = (int)(item - (int64_t)t * slots);
  *x = t < na ? xa + t : xb + (t - na);
  // the rows i of the diagonal: 0 <= i < H and 0 <= j = i + x - dist0 < W
  *shift = *x - dist0;                                 // in [-(H - 1), W - 1]
  const int i_lo = *shift < 0 ? -*shift : 0, i_hi = W - *shift < H ? W - *shift : H;
  const int64_t a64 = (int64_t)i_lo + (int64_t)slot * CHUNK;
  if (a64 >= i_hi) return false;
  *a = (int)a64;
  *b = i_hi - *a > CHUNK ? *a + CHUNK : i_hi;
  return true;
}

// Of the signed diagonals x = dist0 + j - i of the region (a diagonal block: x >= 0) the ones inside the window: xa .. xa + na - 1
// >= 0 and xb .. xb + nb - 1 < 0.  Their distances are one range: the table [d_lo, d_lo + D) must hold it.
struct WindowDiagonals {
  int xa, na, xb, nb;
};
inline int window_diagonals(int H, int W, int diagonal, int64_t dist0, IntWindow win, int64_t d_lo, int64_t D,
                            WindowDiagonals* out) {
  const int64_t w_lo = win.lo, w_hi = win.hi;
  const int64_t x_lo = diagonal ? 0 : dist0 - (H - 1), x_hi = diagonal ? H - 1 : dist0 + (W - 1);
  const int64_t xa = x_lo > w_lo ? x_lo : w_lo, xa_end = x_hi < w_hi ? x_hi : w_hi;
  const int64_t xb = x_lo > -w_hi ? x_lo : -w_hi, xb_end = x_hi < -(w_lo > 1 ? w_lo : 1) ? x_hi : -(w_lo > 1 ? w_lo : 1);
  const int64_t na = xa_end >= xa ? xa_end - xa + 1 : 0, nb = xb_end >= xb ? xb_end - xb + 1 : 0;
  if (na + nb > 0) {
    int64_t lo = INT64_MAX, hi = -1;
    if (na) lo = xa, hi = xa_end;
    if (nb) lo = -xb_end < lo ? -xb_end : lo, hi = -xb > hi ? -xb : hi;
    PHMRF_CHECK(d_lo <= lo && hi < d_lo + D, PHMRF_ERR_INVALID, "the table [d_lo, d_lo + D) does not hold every distance inside the window");
  }
  *out = WindowDiagonals{(int)xa, (int)na, (int)xb, (int)nb};
  return PHMRF_OK;
}

}  // namespace phmrf
