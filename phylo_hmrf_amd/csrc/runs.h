// What the post-processing's kernel files share (smooth.hip, compare.hip, consensus.hip, profile.hip, domains.hip, tracks.hip,
// enrich.hip, enrich_null.hip, pileup.hip, query.hip, aggregate.hip, regrid.hip): the capped grid, the wave helpers of their integer
// accumulations -- one atomic per RUN of equal destination among consecutive lanes, because state maps are piecewise constant
// --, the split of a label row into aligned words (tracks, enrich, enrich_null, query, aggregate, regrid), the order of a wave's LDS
// traffic (query, aggregate, regrid) and the tiles of a distance window (tracks; enrich and enrich_null through enrich_tiles.h), the
// full-matrix area of a grid component, and on the host the owner of a call's device buffers and the
// checks of a region's and a window's arguments (preprocess.hip and render.hip take those too).  What only the interval-list
// kernels share (pileup, query, aggregate) is in interval_lists.h.
#pragma once

#include "common.h"
#include <climits>

namespace phmrf {

inline int grid_of(int64_t n, int tb = 256, int cap = 256 * 16) {
  int64_t g = (n + tb - 1) / tb;
  if (g > cap) g = cap;
  return g < 1 ? 1 : (int)g;
}

__device__ __forceinline__ unsigned long long lanes_at_or_below(int lane) {
  return lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
}

__device__ __forceinline__ void wave_add(unsigned long long* dst, unsigned long long x) {   // one atomic per wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, x);
}

// dst[key] += x, one atomic per run of equal key among consecutive lanes (key < 0: the lane adds nothing).  Every lane of
// the wave must call it.  Inclusive prefix sum, each run's last lane adds the run's part.
template <typename T>
__device__ __forceinline__ void wave_run_add(T* dst, int key, T x) {
  const int lane = threadIdx.x & 63;
  const int key_prev = __shfl_up(key, 1, 64);
  const bool head = lane == 0 || key_prev != key;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T t = __shfl_up(x, off, 64);
    if (lane >= off) x += t;
  }
  const unsigned long long heads = __ballot(head);
  const int h = 63 - __clzll((long long)(heads & lanes_at_or_below(lane)));
  const T before = __shfl(x, h > 0 ? h - 1 : 0, 64);
  const bool next_head = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  if (key >= 0 && next_head) atomicAdd(dst + key, x - (h > 0 ? before : (T)0));
}

// A lane's four keys after a 4-byte load: the run of equal key that starts them goes in through wave_run_add, the keys after
// a change singly; key[e] < 0: the cell adds nothing.  Every lane of the wave must call it.  With x, cell e adds x[e], not 1.
__device__ __forceinline__ void wave_quad_add(unsigned* dst, const int (&key)[4]) {
  unsigned lead = key[0] >= 0 ? 1u : 0u;               // the lane's cells in the bin of its first
  int e = 1;
  for (; e < 4 && lead && key[e] == key[0]; ++e) ++lead;
  wave_run_add(dst, key[0], lead);
  for (; e < 4; ++e)
    if (key[e] >= 0) atomicAdd(dst + key[e], 1u);
}
__device__ __forceinline__ void wave_quad_add(unsigned* dst, const int (&key)[4], const unsigned (&x)[4]) {
  const bool r1 = key[0] >= 0 && key[1] == key[0], r2 = r1 && key[2] == key[0], r3 = r2 && key[3] == key[0];
  const unsigned lead = (key[0] >= 0 ? x[0] : 0u) + (r1 ? x[1] : 0u) + (r2 ? x[2] : 0u) + (r3 ? x[3] : 0u);
  wave_run_add(dst, key[0], lead);
  if (!r1 && key[1] >= 0 && x[1]) atomicAdd(dst + key[1], x[1]);
  if (!r2 && key[2] >= 0 && x[2]) atomicAdd(dst + key[2], x[2]);
  if (!r3 && key[3] >= 0 && x[3]) atomicAdd(dst + key[3], x[3]);
}

// The stored cells of storage row i of a label map between the columns j0 and j1 (a diagonal block: from the diagonal on):
// columns [ja, ja + nc) at p; `head` bytes (at most three) up to the next 4-byte boundary of the address, nvec aligned words of
// four labels, then the bytes from `tail` on: nbytes = head + what follows the words.  A region's slice of a state_vec starts at
// any byte and a diagonal block's rows shift by one node each, so every row has its own head.
struct LabelRow {
  const uint8_t* p;
  int ja, head, nvec, tail, nbytes;
  // the cell, from p, of byte lane q < nbytes: the head bytes first, then the tail's
  __device__ __forceinline__ int byte_at(int q) const { return q < head ? q : tail + (q - head); }
};

__device__ __forceinline__ LabelRow label_row(const uint8_t* __restrict__ labels, int i, int j0, int j1, int W, int diagonal) {
  LabelRow r;
  r.ja = (diagonal && j0 < i) ? i : j0;
  const int nc = j1 - r.ja;                            // >= 1 is the caller's business
  r.p = labels + grid_id<int64_t>(i, r.ja, W, diagonal);
  r.head = (int)((4 - (reinterpret_cast<uintptr_t>(r.p) & 3)) & 3);
  if (r.head > nc) r.head = nc;
  r.nvec = (nc - r.head) >> 2;
  r.tail = r.head + 4 * r.nvec;
  r.nbytes = r.head + (nc - r.tail);
  return r;
}

// lane q's loads of the row (the wave's lane, or the half-wave's where a half-wave holds a row); what it does not hold stays
__device__ __forceinline__ void load_row(const LabelRow& r, int q, uint32_t* word, int* single) {
  if (q < r.nvec) *word = *reinterpret_cast<const uint32_t*>(r.p + r.head + 4 * q);
  if (q < r.nbytes) *single = r.p[r.byte_at(q)];
}

// a wave's LDS traffic in program order for every lane (its histogram is written by some lanes and read by others)
__device__ __forceinline__ void wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// band of a distance d >= 0: 0 for d == 0, else t with 2^(t-1) <= d < 2^t (PHMRF_DIFF_BANDS of them below 2^31)
__device__ __forceinline__ int band_of(long long d) { return d == 0 ? 0 : 64 - __clzll(d); }

// the area on the full matrix of the component with root v, from acc[v] = (weight << 32) | nodes (weight: 1 per diagonal
// node, 2 per other node) and mirror[v] = a node has j - i <= 1: a diagonal block's component that is its own mirror counts
// its off-diagonal nodes twice, any other component its stored nodes
__device__ __forceinline__ long long component_area(int64_t v, int diagonal, const unsigned long long* __restrict__ acc,
                                                    const uint8_t* __restrict__ mirror) {
  const unsigned long long a = acc[v];
  return (diagonal && mirror[v]) ? (long long)(a >> 32) : (long long)(a & 0xffffffffull);
}

// a finite float32 in [0, 1], told by its bits (the library is compiled with -fno-honor-nans: a comparison proves nothing
// about a NaN): +0 .. 1.0 are the patterns up to 0x3f800000, and -0
__host__ __device__ __forceinline__ bool unit_bits(uint32_t u) { return u <= 0x3f800000u || u == 0x80000000u; }
__device__ __forceinline__ bool unit_conf(float c) { return unit_bits(__float_as_uint(c)); }

// rows [i0, i1) and columns [j0, j1) of the storage; whole: every cell is inside the distance window; the cells' distances
// lie in [near, near + nd)
struct WindowTile {
  int i0, i1, j0, j1, near, nd;
  bool whole;
};

// Tile T of a region cut into tiles of TILE_H storage rows by TILE_W storage columns, per_row of them side by side (a
// diagonal block: the upper triangle of the per_row x per_row grid of TILE_W-square super-tiles, TILE_W / TILE_H tiles each);
// false for a tile of the last super-tile row's padding, and for a tile wholly outside the window d_lo <= |dist0 + j - i|
// <= d_hi (the same answer for the whole workgroup)
template <int TILE_H, int TILE_W>
__device__ __forceinline__ bool window_tile(int64_t T, int H, int W, int diagonal, int per_row, int dist0, int d_lo, int d_hi,
                                            WindowTile* t) {
  constexpr int PER_SUPER = TILE_W / TILE_H;
  int ti, tj;
  if (diagonal) {
    int g;
    grid_coords(T / PER_SUPER, per_row, 1, &g, &tj);
    ti = g * PER_SUPER + (int)(T % PER_SUPER);
  } else {
    grid_coords(T, per_row, 0, &ti, &tj);
  }
  const int64_t i0 = (int64_t)ti * TILE_H;
  if (i0 >= H) return false;
  int64_t j0 = (int64_t)tj * TILE_W;
  const int64_t i1 = i0 + TILE_H < H ? i0 + TILE_H : H;
  const int64_t j1 = j0 + TILE_W < W ? j0 + TILE_W : W;
  t->i0 = (int)i0;
  t->i1 = (int)i1;
  t->j0 = (int)j0;
  t->j1 = (int)j1;
  if (diagonal && j0 < i0) j0 = i0;                    // the stored cells of the tile start at the diagonal
  if (j0 >= j1) return false;
  // the range of dist0 + j - i over the tile (|dist0| + H + W < 2^31: an int holds every distance)
  const int x_lo = dist0 + (int)j0 - ((int)i1 - 1), x_hi = dist0 + ((int)j1 - 1) - (int)i0;
  const int a_lo = x_lo < 0 ? -x_lo : x_lo, a_hi = x_hi < 0 ? -x_hi : x_hi;
  const int far = a_lo > a_hi ? a_lo : a_hi;
  const int near = (x_lo <= 0 && x_hi >= 0) ? 0 : (a_lo < a_hi ? a_lo : a_hi);
  if (far < d_lo || near > d_hi) return false;
  t->whole = near >= d_lo && far <= d_hi;
  t->near = near;
  t->nd = far - near + 1;                              // <= x_hi - x_lo + 1 <= TILE_H + TILE_W - 1
  return true;
}

// The rows i0 + first, + STEP, ... of tile t, one to an entry of word / single, as lane q of the lanes that hold a row reads
// them: every load of the tile is issued before the first count.  An absent row, and what a lane does not hold of a row, is 0.
template <int STEP, int N>
__device__ __forceinline__ void load_tile_rows(const uint8_t* __restrict__ labels, const WindowTile& t, int W, int diagonal, int first,
                                               int q, uint32_t (&word)[N], int (&single)[N]) {
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int i = t.i0 + first + STEP * u;
    word[u] = 0;
    single[u] = 0;                                     // (nc >= 1 below: a diagonal block's tile ends right of the diagonal)
    if (i < t.i1) load_row(label_row(labels, i, t.j0, t.j1, W, diagonal), q, &word[u], &single[u]);
  }
}

// ---- what the entry points share on the host ---------------------------------------------------------------------------

// The device allocations of one call, freed on every way out.
class Buffers {
 public:
  Buffers() = default;
  Buffers(const Buffers&) = delete;
  Buffers& operator=(const Buffers&) = delete;
  ~Buffers() {
    for (void* p : owned_) (void)hipFree(p);
  }
  template <typename T>
  int get(T** p, size_t count) {                       // *p = max(count, 1) elements
    PHMRF_HIP(hipMalloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T)));
    owned_.push_back(*p);
    return PHMRF_OK;
  }
  template <typename T>
  int release(T** p) {                                 // frees *p (null: nothing to do) ahead of time, to get it again larger
    for (size_t t = 0; t < owned_.size(); ++t)
      if (*p && owned_[t] == *p) {
        owned_.erase(owned_.begin() + t);
        PHMRF_HIP(hipFree(*p));
        break;
      }
    *p = nullptr;
    return PHMRF_OK;
  }

 private:
  std::vector<void*> owned_;
};

// H, W >= 1, diagonal in {0, 1}, a diagonal block square; *n = the region's stored nodes
inline int check_region(int H, int W, int diagonal, int64_t* n = nullptr) {
  PHMRF_CHECK(H >= 1 && W >= 1, PHMRF_ERR_INVALID, "H and W must be >= 1");
  PHMRF_CHECK(diagonal == 0 || diagonal == 1, PHMRF_ERR_INVALID, "diagonal must be 0 or 1");
  PHMRF_CHECK(!diagonal || H == W, PHMRF_ERR_INVALID, "a diagonal block is square (H == W)");
  if (n) *n = grid_row_first<int64_t>(H, W, diagonal);
  return PHMRF_OK;
}

// the states of one map (KB: a second map's, `names` then says "KA and KB")
inline int check_states(int K, int KB = 1, const char* names = "K") {
  PHMRF_CHECK(K >= 1 && KB >= 1, PHMRF_ERR_INVALID, std::string(names) + " must be >= 1");
  PHMRF_CHECK(K <= 64 && KB <= 64, PHMRF_ERR_UNSUPPORTED, std::string(names) + " must be <= 64");
  return PHMRF_OK;
}

// node ids and the 64 past the last that a wave may form fit an int
inline int check_nodes(int64_t n, const char* msg = "the region must have fewer than 2^31 - 64 nodes") {
  PHMRF_CHECK(n < ((int64_t)1 << 31) - 64, PHMRF_ERR_UNSUPPORTED, msg);
  return PHMRF_OK;
}

inline int check_window(int64_t d_min, int64_t d_max) {
  PHMRF_CHECK(d_min >= 0, PHMRF_ERR_INVALID, "d_min must be >= 0");
  PHMRF_CHECK(d_max == -1 || d_max >= d_min, PHMRF_ERR_INVALID, "d_max must be >= d_min, or -1 for no upper limit");
  return PHMRF_OK;
}

// an int holds dist0 + j - i of every cell of an H x W region and of a tile's padding (window_tile)
inline int check_span(int64_t dist0, int H, int W) {
  PHMRF_CHECK(dist0 > -((int64_t)1 << 31) && (dist0 < 0 ? -dist0 : dist0) + H + W < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED,
              "|dist0| + H + W must be below 2^31");
  return PHMRF_OK;
}

// the window for the kernels.  Every distance is below INT_MAX: a d_min up there leaves nothing inside, a d_max up there is none
struct IntWindow {
  int lo, hi;
};
inline IntWindow int_window(int64_t d_min, int64_t d_max) {
  return IntWindow{d_min < INT_MAX ? (int)d_min : INT_MAX, (d_max == -1 || d_max > INT_MAX) ? INT_MAX : (int)d_max};
}

// the tiles window_tile<TILE_H, TILE_W> enumerates over an H x W region, and how many lie side by side
template <int TILE_H, int TILE_W>
inline int64_t window_tile_count(int H, int W, int diagonal, int* per_row) {
  constexpr int PER_SUPER = TILE_W / TILE_H;
  *per_row = (W + TILE_W - 1) / TILE_W;
  return diagonal ? (int64_t)PER_SUPER * grid_row_first<int64_t>(*per_row, *per_row, 1)
                  : (int64_t)((H + TILE_H - 1) / TILE_H) * *per_row;
}

// every distance |dist0 + j - i| of an H x W region is below 2^31 (band_of, the int distances of domains.hip)
inline int check_reach(int64_t dist0, int H, int W, const char* suffix = " has no band") {
  const int64_t reach = (dist0 < 0 ? -dist0 : dist0) + (H > W ? H : W);
  PHMRF_CHECK(dist0 > -((int64_t)1 << 31) && reach < ((int64_t)1 << 31), PHMRF_ERR_INVALID,
              std::string("a distance |dist0 + j - i| of 2^31 or more") + suffix);
  return PHMRF_OK;
}

}  // namespace phmrf
