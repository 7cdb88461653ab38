// What the kernels that count a state map under a LIST of intervals share (pileup.hip, query.hip, aggregate.hip; DESIGN.md
// section 7; regrid.hip takes the first, the second and the last): the limit of a coordinate, the clip of a rectangle to a
// region, the table of the groups' entries and chunks (pileup, aggregate; each kernel decomposes its items itself), a lane's
// private LDS column of 16-bit counters (pileup, aggregate) and, on the host, the zeroed output table with the flag word
// behind it (all three, and regrid).  Integers only.
#pragma once

#include "runs.h"

namespace phmrf {

constexpr int MAX_GROUPS = 16;           // G <= 16 (intervals.py MAX_GROUPS)
constexpr int COORD_LIMIT = 1 << 30;     // a coordinate has |c| < 2^30: sums and differences of two stay in an int

// the one range test of a coordinate: true for a c that is refused
template <typename T>
__host__ __device__ __forceinline__ bool coord_out(T c) {
  return c <= -COORD_LIMIT || c >= COORD_LIMIT;
}

// rows [x0, x1) and columns [y0, y1), local to an H x W region, clipped to it (a diagonal block: to its upper triangle, so
// that i1 <= j1 and every row holds a stored cell); false: nothing stored there
__host__ __device__ __forceinline__ bool clip_rect(int H, int W, int diagonal, long long x0, long long x1, long long y0, long long y1,
                                                   int* i0, int* i1, int* j0, int* j1) {
  if (x0 < 0) x0 = 0;
  if (x1 > H) x1 = H;
  if (y0 < 0) y0 = 0;
  if (y1 > W) y1 = W;
  if (diagonal && x1 > y1) x1 = y1;                    // a row at or below y1 holds no stored cell of the rectangle
  if (x0 >= x1 || y0 >= y1) return false;
  *i0 = (int)x0;
  *i1 = (int)x1;
  *j0 = (int)y0;
  *j1 = (int)y1;
  return true;
}

// first[g] .. first[g + 1]: the entries of group g; chunk0[g]: the first chunk of group g, chunk0[G] the number of chunks.
// Both repeat their last value past G.  The table travels in the kernel's arguments.
struct GroupChunks {
  long long first[MAX_GROUPS + 1];
  long long chunk0[MAX_GROUPS + 1];
};

// fills first[] from the G + 1 offsets (G <= MAX_GROUPS is the caller's check); *total = the entries, `noun` names them
inline int group_first(const int64_t* offsets, int G, const char* noun, GroupChunks* gr, int64_t* total) {
  PHMRF_CHECK(offsets[0] == 0, PHMRF_ERR_INVALID, "the group offsets must start at 0");
  for (int g = 0; g <= MAX_GROUPS; ++g) {
    const int64_t at = offsets[g < G ? g : G];
    PHMRF_CHECK(g == 0 || g > G || at >= offsets[g - 1], PHMRF_ERR_INVALID, "the group offsets must not decrease");
    gr->first[g] = at;
  }
  *total = offsets[G];
  PHMRF_CHECK(*total < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED, std::string("there must be fewer than 2^31 ") + noun);
  return PHMRF_OK;
}

// fills chunk0[] for chunks of at most `len` entries of one group
inline void group_chunks(GroupChunks* gr, int len) {
  gr->chunk0[0] = 0;
  for (int g = 0; g < MAX_GROUPS; ++g) gr->chunk0[g + 1] = gr->chunk0[g] + (gr->first[g + 1] - gr->first[g] + len - 1) / len;
}

// the group of entry f
__device__ __forceinline__ int group_of_entry(const GroupChunks& gr, int64_t f) {
  int g = 0;
  while (g < MAX_GROUPS - 1 && gr.first[g + 1] <= f) ++g;
  return g;
}

// A lane's PRIVATE column of counters in LDS, laid out [k / 2][lane] over the LANES lanes of a workgroup: 16 bits a state, two
// states to a u32 word (that no counter carries is the kernel's business).  A lane only ever touches its own column, whose
// words fall on bank lane mod 32 of its half-wave: no LDS atomics, no bank conflicts and no barrier.
template <int LANES>
__device__ __forceinline__ void packed_bump(unsigned* col, int s) {
  col[(s >> 1) * LANES] += 1u << (16 * (s & 1));
}

// adds the non-zero counters of a column of `words` words to out[0 .. 2 words) with u64 atomics and zeroes them
template <int LANES>
__device__ __forceinline__ void packed_flush(unsigned* col, int words, unsigned long long* out) {
  for (int q = 0; q < words; ++q) {
    const unsigned n = col[q * LANES];
    if (n) {
      if (n & 0xffffu) atomicAdd(out + 2 * q, (unsigned long long)(n & 0xffffu));
      if (n >> 16) atomicAdd(out + 2 * q + 1, (unsigned long long)(n >> 16));        // (K odd: the last word's high half stays 0)
      col[q * LANES] = 0;
    }
  }
}

// The u64 output words of a call and, behind them, the flag word its kernels OR their findings into: one allocation and one
// memset.  The words hold counts below 2^63 and go to the caller's int64 tables as they are.
class FlaggedTable {
 public:
  explicit FlaggedTable(hipStream_t st) : st_(st) {}
  bool made() const { return words_ != nullptr; }
  int make(Buffers* buf, size_t n) {                   // n zeroed words | the zeroed flag word
    n_ = n;
    PHMRF_TRY(buf->get(&words_, n + 1));
    PHMRF_HIP(hipMemsetAsync(words_, 0, (n + 1) * sizeof(unsigned long long), st_));
    return PHMRF_OK;
  }
  unsigned long long* words() const { return words_; }
  int* flag() const { return reinterpret_cast<int*>(words_ + n_); }
  int read_flag(int* bad) const {                      // waits for the kernels
    PHMRF_HIP(hipMemcpyAsync(bad, flag(), sizeof(int), hipMemcpyDeviceToHost, st_));
    PHMRF_HIP(hipStreamSynchronize(st_));
    return PHMRF_OK;
  }
  int copy(size_t offset, size_t count, int64_t* host) const {      // asynchronous: wait() after the last
    static_assert(sizeof(int64_t) == sizeof(unsigned long long), "the tables are copied as they are");
    PHMRF_HIP(hipMemcpyAsync(host, words_ + offset, count * sizeof(unsigned long long), hipMemcpyDeviceToHost, st_));
    return PHMRF_OK;
  }
  int wait() const {
    PHMRF_HIP(hipStreamSynchronize(st_));
    return PHMRF_OK;
  }

 private:
  hipStream_t st_;
  unsigned long long* words_ = nullptr;
  size_t n_ = 0;
};

}  // namespace phmrf
