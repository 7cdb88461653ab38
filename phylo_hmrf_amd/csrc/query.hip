// gfx950 kernel that counts the states inside many rectangles of ONE region's state map (phmrf_rect_states; DESIGN.md
// section 7): counts[slot][k] += +-(the stored nodes of the rectangle in state k), conf[slot] += +-(their confidences in 2^-24
// fixed point).  Integer arithmetic throughout: no result depends on the order in which the atomics land.
//
//   The entry point clips every rectangle to the region (a diagonal block: to its upper triangle) on the host, drops the empty
//   ones and cuts the rest into ITEMS of at most RECT_TILE_H storage rows by RECT_TILE_W storage columns; the items of one
//   rectangle are consecutive, in a diagonal block every row band starts its items at the diagonal, and an item wholly below
//   the diagonal is never made.  The item table is uploaded in batches of at most RECT_BATCH items; one kernel per batch.
//   One WAVE takes one item at a time (the waves of the capped grid stride over the table; the four waves of a workgroup share
//   nothing and meet at no barrier).  The lanes walk the item's cells row-major, so a run of equal state within a storage row
//   is a run of consecutive lanes:
//     an item of fewer than RECT_VEC_MIN columns is walked as ONE sequence of rows x columns cells, a byte per lane (a loop
//     anchor of 3 x 3 bins is one step of nine lanes, not three steps of three);
//     a wider item goes row by row through label_row (runs.h): up to three head bytes, one aligned 4-byte word of four labels
//     per lane, up to three tail bytes.
//   Every wave keeps a private histogram of K u32 bins in LDS (an item has at most 4,096 cells: a bin never carries) and adds
//   to it with wave_run_add, one LDS atomic per run; a lane's confidences are summed in a register.  After the item K
//   consecutive lanes add the non-zero bins to K consecutive words of counts[slot] with u64 global atomics and zero them; a
//   subtracted rectangle adds the two's complement.  The confidence sum is reduced over the wave and added once.
//   Only a node that some rectangle holds is looked at.  Flag bits: a label >= K on such a node, a confidence there that is no
//   finite number in [0, 1].  Coordinates, slots and signs are checked on the host, where the rectangles are clipped.

#include "interval_lists.h"

namespace phmrf {
namespace {

constexpr int RECT_TILE_H = 16;          // storage rows of an item (query.py TILE_H)
constexpr int RECT_TILE_W = 256;         // storage columns of an item: at most one 4-byte word a lane (query.py TILE_W)
constexpr int RECT_VEC_MIN = 32;         // an item of at least this many columns is read in aligned words (query.py VEC_MIN)
constexpr int RECT_WAVES = 4;            // waves of a workgroup, one item each (query.py WAVES)
constexpr int RECT_GRID_CAP = 2048;      // workgroups (query.py GRID_CAP)
constexpr int64_t RECT_BATCH = 1 << 20;  // items uploaded and launched together (query.py BATCH)
constexpr int BAD_LABEL = 1, BAD_CONF = 2;

static_assert(RECT_TILE_W == 4 * 64, "a row of an item is at most one word per lane");
static_assert((int64_t)RECT_TILE_H * RECT_TILE_W < ((int64_t)1 << 32), "a u32 bin holds an item");

// rows [i0, i1) and columns [j0, j1) of the storage, all inside the region; in a diagonal block i1 <= j1, so that every row
// holds a stored cell, and the cells left of the diagonal are passed over
struct RectItem {
  int32_t i0, i1, j0, j1, slot, minus;
};

// counts: u64 [Q][K]; conf_sum: u64 [Q]
__global__ __launch_bounds__(64 * RECT_WAVES) void rect_states_kernel(const uint8_t* __restrict__ labels, const float* __restrict__ conf,
                                                                     int W, int diagonal, int K, const RectItem* __restrict__ items,
                                                                     int64_t nitems, unsigned long long* __restrict__ counts,
                                                                     unsigned long long* __restrict__ conf_sum, int* __restrict__ bad) {
  __shared__ unsigned hist_all[RECT_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* const hist = hist_all[wave];
  hist[lane] = 0;
  wave_order();
  int wrong = 0;
  // one cell: the state, or -1 for a label >= K; its confidence goes into f
  auto cell = [&](int s, int64_t v, unsigned long long& f) -> int {
    if (s >= K) {
      wrong |= BAD_LABEL;
      return -1;
    }
    if (conf) {
      const float c = conf[v];
      if (unit_conf(c))
        f += (unsigned long long)(c * 16777216.0f);      // exact: a float32 in [0, 1] times 2^24
      else
        wrong |= BAD_CONF;
    }
    return s;
  };
  for (int64_t t = (int64_t)blockIdx.x * RECT_WAVES + wave; t < nitems; t += (int64_t)gridDim.x * RECT_WAVES) {
    const RectItem it = items[t];                        // (the same for every lane)
    const int w = it.j1 - it.j0, nr = it.i1 - it.i0;
    unsigned long long f = 0;
    if (w < RECT_VEC_MIN) {
      const int cells = nr * w;                          // < 16 * 32
      for (int c0 = 0; c0 < cells; c0 += 64) {
        const int c = c0 + lane;
        int key = -1;
        if (c < cells) {
          const int r = c / w, i = it.i0 + r, j = it.j0 + (c - r * w);
          if (!diagonal || j >= i) {
            const int64_t v = grid_id<int64_t>(i, j, W, diagonal);
            key = cell(labels[v], v, f);
          }
        }
        wave_run_add(hist, key, key >= 0 ? 1u : 0u);
      }
    } else {
      for (int i = it.i0; i < it.i1; ++i) {
        const LabelRow r = label_row(labels, i, it.j0, it.j1, W, diagonal);       // (nc >= 1: i < i1 <= j1 in a diagonal block)
        const int64_t v0 = r.p - labels;
        uint32_t word = 0;
        int single = 0;
        load_row(r, lane, &word, &single);
        if (r.nvec > 0) {
          int key[4] = {-1, -1, -1, -1};
          if (lane < r.nvec) {
#pragma unroll
            for (int e = 0; e < 4; ++e) key[e] = cell((int)((word >> (8 * e)) & 0xff), v0 + r.head + 4 * lane + e, f);
          }
          wave_quad_add(hist, key);
        }
        if (r.nbytes > 0) {
          int key = -1;
          if (lane < r.nbytes) key = cell(single, v0 + r.byte_at(lane), f);
          wave_run_add(hist, key, key >= 0 ? 1u : 0u);
        }
      }
    }
    wave_order();
    if (lane < K) {
      const unsigned n = hist[lane];
      if (n) {
        atomicAdd(counts + (int64_t)it.slot * K + lane, it.minus ? 0ull - (unsigned long long)n : (unsigned long long)n);
        hist[lane] = 0;
      }
    }
    wave_order();
    if (conf) wave_add(conf_sum + it.slot, it.minus ? 0ull - f : f);    // (a wave whose sum is 0 adds nothing)
  }
  if (wrong) atomicOr(bad, wrong);
}

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_rect_states(const uint8_t* labels_dev, const float* conf_dev_or_null, int H, int W, int diagonal, int K, int64_t R,
                      const int32_t* rect_host, const int32_t* slot_host_or_null, const uint8_t* minus_host_or_null, int64_t Q,
                      int64_t* counts_host, int64_t* conf_host_or_null, void* hip_stream) {
  PHMRF_CHECK(labels_dev && counts_host, PHMRF_ERR_INVALID, "NULL labels or output table");
  PHMRF_CHECK(R >= 0, PHMRF_ERR_INVALID, "R must be >= 0");
  PHMRF_CHECK(rect_host || R == 0, PHMRF_ERR_INVALID, "NULL rectangles");
  PHMRF_CHECK(!conf_host_or_null || conf_dev_or_null, PHMRF_ERR_INVALID, "a confidence table without confidences");
  int64_t n = 0;
  PHMRF_TRY(check_region(H, W, diagonal, &n));
  PHMRF_CHECK(K >= 1, PHMRF_ERR_INVALID, "K must be >= 1");
  PHMRF_CHECK(Q >= 1, PHMRF_ERR_INVALID, "Q must be >= 1");
  PHMRF_CHECK(slot_host_or_null || Q == R, PHMRF_ERR_INVALID, "without slots Q must be R");
  PHMRF_TRY(check_states(K));
  PHMRF_TRY(check_nodes(n, "n must be below 2^31 - 64"));
  PHMRF_CHECK(R < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED, "there must be fewer than 2^31 rectangles");
  PHMRF_CHECK(Q < ((int64_t)1 << 31) && Q * K < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED, "Q K must be below 2^31");
  for (int64_t t = 0; t < R; ++t) {                      // every rectangle is checked before the first is counted
    PHMRF_CHECK(!slot_host_or_null || (slot_host_or_null[t] >= 0 && slot_host_or_null[t] < Q), PHMRF_ERR_INVALID,
                "a slot is outside [0, Q)");
    PHMRF_CHECK(!minus_host_or_null || minus_host_or_null[t] <= 1, PHMRF_ERR_INVALID, "a minus byte is > 1");
  }
  for (int64_t t = 0; t < 4 * R; ++t)
    PHMRF_CHECK(!coord_out(rect_host[t]), PHMRF_ERR_UNSUPPORTED, "a rectangle coordinate has |c| >= 2^30");

  const size_t n_counts = (size_t)Q * K;                 // the table: counts | confidence sums
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  Buffers buf;
  FlaggedTable tab(st);
  RectItem* items_dev = nullptr;
  int64_t items_cap = 0;
  std::vector<RectItem> items;
  // uploads the items gathered so far and counts them; the first call makes the device tables
  auto flush = [&]() -> int {
    if (items.empty()) return PHMRF_OK;
    if (!tab.made()) PHMRF_TRY(tab.make(&buf, n_counts + (size_t)Q));
    const int64_t m = (int64_t)items.size();
    if (m > items_cap) {                                 // (only a call's last batch is smaller than its first)
      PHMRF_TRY(buf.release(&items_dev));
      PHMRF_TRY(buf.get(&items_dev, (size_t)m));
      items_cap = m;
    }
    PHMRF_HIP(hipMemcpyAsync(items_dev, items.data(), (size_t)m * sizeof(RectItem), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(rect_states_kernel, dim3(grid_of(m, RECT_WAVES, RECT_GRID_CAP)), dim3(64 * RECT_WAVES), 0, st, labels_dev,
                       conf_dev_or_null, W, diagonal, K, items_dev, m, tab.words(), tab.words() + n_counts, tab.flag());
    PHMRF_HIP(hipGetLastError());
    PHMRF_HIP(hipStreamSynchronize(st));                 // the host vector and the device table are taken again
    items.clear();
    return PHMRF_OK;
  };
  for (int64_t t = 0; t < R; ++t) {
    int i0, i1, j0, j1;
    if (!clip_rect(H, W, diagonal, rect_host[4 * t], rect_host[4 * t + 1], rect_host[4 * t + 2], rect_host[4 * t + 3], &i0, &i1, &j0, &j1))
      continue;
    const int32_t slot = slot_host_or_null ? slot_host_or_null[t] : (int32_t)t;
    const int32_t minus = minus_host_or_null ? minus_host_or_null[t] : 0;
    for (int a = i0; a < i1; a += RECT_TILE_H) {
      const int a1 = a + RECT_TILE_H < i1 ? a + RECT_TILE_H : i1;
      for (int b = (diagonal && j0 < a) ? a : j0; b < j1; b += RECT_TILE_W) {        // (a < i1 <= j1 in a diagonal block)
        const int b1 = b + RECT_TILE_W < j1 ? b + RECT_TILE_W : j1;
        items.push_back(RectItem{a, (diagonal && a1 > b1) ? b1 : a1, b, b1, slot, minus});
        if ((int64_t)items.size() == RECT_BATCH) PHMRF_TRY(flush());
      }
    }
  }
  PHMRF_TRY(flush());
  if (!tab.made()) {                                     // no rectangle holds a node
    for (size_t x = 0; x < n_counts; ++x) counts_host[x] = 0;
    if (conf_host_or_null)
      for (int64_t q = 0; q < Q; ++q) conf_host_or_null[q] = 0;
    return PHMRF_OK;
  }
  int bad = 0;
  PHMRF_TRY(tab.read_flag(&bad));
  PHMRF_CHECK(!(bad & BAD_LABEL), PHMRF_ERR_INVALID, "a label inside a rectangle is >= K");
  PHMRF_CHECK(!(bad & BAD_CONF), PHMRF_ERR_INVALID, "a confidence inside a rectangle is not a finite number in [0, 1]");
  PHMRF_TRY(tab.copy(0, n_counts, counts_host));
  if (conf_host_or_null) PHMRF_TRY(tab.copy(n_counts, (size_t)Q, conf_host_or_null));
  return tab.wait();
}

}  // extern "C"
