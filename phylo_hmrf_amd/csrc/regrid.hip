// gfx950 kernels that resample ONE chromosome's state map onto ONE region of another grid (phmrf_regrid_states; DESIGN.md
// section 7).  The source has bins of a units and the target bins of b units, gcd(a, b) = 1: source bin p covers the units
// [p a, (p + 1) a), target bin x the units [x b, (x + 1) b), ov(x, p) = the units they share.  Target cell (x, y) takes from every
// stored node (p, q) of every source region in state k
//   votes[x][y][k] += ov(x, p) ov(y, q) + [p != q] ov(x, q) ov(y, p):
// the symmetric chromosome matrix read through all its regions, exactly across seams and through mirror halves.  The host has
// refused source regions that overlap on the full matrix, so covered = sum_k votes <= b^2 <= 2^30 and every count is a u32.
// Integer arithmetic throughout: no result depends on the order in which the atomics land.
//
//   Axis tables (host): per target row and per target column of the region the first source bin p0, the number n of source
//   bins and the first and the last overlap weight; a bin between the two lies wholly inside the target bin and weighs a
//   (n >= 3 only when a < b).  No lane divides.
//   Piece table (host): every source region is cut against the source bins the target region reads, once as it is stored
//   (rows x columns) and once mirrored (columns x rows); the kernels walk the non-empty pieces, at most 2 R.  A mirrored
//   piece is read along the source's storage rows like a direct one, its nodes with p == q left out.
//   Two regimes, by the largest source rectangle of a target cell, nmax^2 with nmax = 1 + ceil((b - 1) / a):
//   regrid_lane_kernel (nmax^2 <= REGRID_SMALL_AREA): a lane per target cell, REGRID_LANES consecutive stored target nodes a
//   workgroup; neighbouring lanes read neighbouring bytes of a source row.  While a cell has met one state only it keeps
//   the sum in a register; with the second state it moves to a PRIVATE column of u32 counters in LDS, [k][lane].
//   regrid_wave_kernel (above): a wave per target cell.  It walks every clipped rectangle row by row in pieces of at most 256
//   columns through label_row / wave_quad_add (runs.h) into a private u32 histogram in LDS; one wave reduction gives the
//   arg-max, the lowest state on ties.
//   Both write state, support and covered of every stored target cell into the call's scratch planes; the host copies them to
//   the caller's only when no label >= K was met inside a read cell.

#include "interval_lists.h"

namespace phmrf {
namespace {

constexpr int REGRID_LANES = 128;          // target cells of a tile = lanes of a workgroup of the lane kernel (regrid.py LANES)
constexpr int REGRID_GRID_CAP = 4096;      // workgroups of the lane kernel (regrid.py GRID_CAP)
constexpr int REGRID_SMALL_AREA = 256;     // nmax^2 above this: a wave per target cell (regrid.py SMALL_AREA; unmeasured)
constexpr int REGRID_WAVES = 4;            // waves of a workgroup of the wave kernel (regrid.py WAVES)
constexpr int REGRID_WAVE_GRID_CAP = 2048; // workgroups of the wave kernel (regrid.py WAVE_GRID_CAP)
constexpr int REGRID_ROW_W = 256;          // columns of a row piece: at most one 4-byte word a lane (regrid.py ROW_W)
constexpr int REGRID_MAX_REGIONS = 64;     // R <= 64 (regrid.py MAX_REGIONS)
constexpr int REGRID_MAX_RATIO = 1 << 15;  // a, b <= 2^15: b^2 <= 2^30 (regrid.py MAX_RATIO)

static_assert(REGRID_ROW_W == 4 * 64, "a row piece is at most one word per lane");
static_assert((int64_t)REGRID_MAX_RATIO * REGRID_MAX_RATIO <= ((int64_t)1 << 30), "a u32 holds a cell's votes");

// a non-empty piece of a source region: storage rows [i0, i1) and columns [j0, j1) of the region whose slice starts at lo
struct RegridPiece {
  long long lo;
  int W, diagonal, s1, s2, i0, i1, j0, j1, mirror, pad;
};

// a target row or column: the source bins [p0, p0 + n) with the weights wf, inner ..., wl (n == 1: wf)
struct RegridAxis {
  long long p0;
  int n, wf, wl, pad;
};

struct RegridTarget {
  int H, W, diagonal, K, inner;            // inner = a: the weight of a source bin wholly inside a target bin
  unsigned min_cover;
  int fill, npieces;
  long long n_t;
};

__device__ __forceinline__ unsigned regrid_weight(const RegridAxis& ax, long long t, int inner) {
  return t == 0 ? (unsigned)ax.wf : (t == ax.n - 1 ? (unsigned)ax.wl : (unsigned)inner);
}

// stored target node v -> its row and column in the region
__device__ __forceinline__ void regrid_cell(long long v, const RegridTarget& tg, int* r, int* c) {
  if (tg.diagonal) {
    grid_coords(v, tg.W, 1, r, c);
  } else {
    *r = (int)((unsigned)v / (unsigned)tg.W);          // v < 2^31: a 32-bit division
    *c = (int)((unsigned)v - (unsigned)*r * (unsigned)tg.W);
  }
}

// the stored cells of piece pc that the target cell with the axes ax (row) and ay (column) reads; false: none
__device__ __forceinline__ bool regrid_clip(const RegridPiece& pc, const RegridAxis& ax, const RegridAxis& ay, int* i0, int* i1,
                                            int* j0, int* j1) {
  const RegridAxis& rows = pc.mirror ? ay : ax;
  const RegridAxis& cols = pc.mirror ? ax : ay;
  long long x0 = rows.p0 - pc.s1, x1 = x0 + rows.n, y0 = cols.p0 - pc.s2, y1 = y0 + cols.n;
  if (x0 < pc.i0) x0 = pc.i0;
  if (x1 > pc.i1) x1 = pc.i1;
  if (y0 < pc.j0) y0 = pc.j0;
  if (y1 > pc.j1) y1 = pc.j1;
  if (pc.diagonal && x1 > y1) x1 = y1;                 // a row at or below y1 holds no stored cell of the rectangle
  if (x0 >= x1 || y0 >= y1) return false;
  *i0 = (int)x0;
  *i1 = (int)x1;
  *j0 = (int)y0;
  *j1 = (int)y1;
  return true;
}

// the call's output for one cell
__device__ __forceinline__ void regrid_store(long long v, int state, unsigned sup, unsigned cov, uint8_t* __restrict__ state_out,
                                             unsigned* __restrict__ support, unsigned* __restrict__ covered) {
  state_out[v] = (uint8_t)state;
  if (support) support[v] = sup;
  if (covered) covered[v] = cov;
}

// hist: u64 [K + 1] (hist[K]: the uncalled cells), then the mixed cells
__global__ __launch_bounds__(REGRID_LANES) void regrid_lane_kernel(const uint8_t* __restrict__ labels,
                                                                   const RegridPiece* __restrict__ pieces,
                                                                   const RegridAxis* __restrict__ rows,
                                                                   const RegridAxis* __restrict__ cols, RegridTarget tg, int64_t ntiles,
                                                                   uint8_t* __restrict__ state_out, unsigned* __restrict__ support,
                                                                   unsigned* __restrict__ covered, unsigned long long* __restrict__ hist,
                                                                   int* __restrict__ bad) {
  extern __shared__ unsigned regrid_cols[];            // [K][REGRID_LANES] u32: a lane's column is private
  unsigned* const col = regrid_cols + threadIdx.x;
  const int K = tg.K;
  for (int k = 0; k < K; ++k) col[k * REGRID_LANES] = 0;
  int wrong = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long v = (long long)tile * REGRID_LANES + threadIdx.x;
    int key = -1;
    unsigned long long is_mixed = 0;
    if (v < tg.n_t) {
      int r, c;
      regrid_cell(v, tg, &r, &c);
      const RegridAxis ax = rows[r], ay = cols[c];
      unsigned total = 0;
      int first = -1;
      bool many = false;                               // a second state was met: the counts are in the column
      for (int t = 0; t < tg.npieces; ++t) {
        const RegridPiece pc = pieces[t];
        int i0, i1, j0, j1;
        if (!regrid_clip(pc, ax, ay, &i0, &i1, &j0, &j1)) continue;
        const uint8_t* const lab = labels + pc.lo;
        for (int i = i0; i < i1; ++i) {
          const int ja = (pc.diagonal && j0 < i) ? i : j0;                           // (i < i1 <= j1 in a diagonal block)
          const uint8_t* const p = lab + grid_id<int64_t>(i, ja, pc.W, pc.diagonal);
          const long long bin_i = (long long)pc.s1 + i;
          const long long same = pc.mirror ? bin_i - pc.s2 : -1;                     // the column of the bin pair (p, p)
          const unsigned wi = pc.mirror ? regrid_weight(ay, bin_i - ay.p0, tg.inner) : regrid_weight(ax, bin_i - ax.p0, tg.inner);
          const RegridAxis& other = pc.mirror ? ax : ay;
          for (int j = ja; j < j1; ++j) {
            if (j == same) continue;
            const int s = p[j - ja];
            if (s >= K) {
              wrong = 1;
              continue;
            }
            const unsigned w = wi * regrid_weight(other, (long long)pc.s2 + j - other.p0, tg.inner);
            total += w;
            if (!many) {
              if (first < 0) first = s;
              else if (s != first) {
                col[first * REGRID_LANES] = total - w;
                many = true;
              }
            }
            if (many) col[s * REGRID_LANES] += w;
          }
        }
      }
      unsigned best_n = total;
      int best = first < 0 ? 0 : first;
      if (many) {
        best_n = 0;
        best = 0;
        for (int k = 0; k < K; ++k) {                  // ascending states and a strict >: the lowest state wins a tie
          const unsigned n = col[k * REGRID_LANES];
          if (n > best_n) {
            best_n = n;
            best = k;
          }
          col[k * REGRID_LANES] = 0;
        }
      }
      const bool called = total >= tg.min_cover;
      key = called ? best : K;
      is_mixed = (called && best_n < total) ? 1ull : 0ull;
      regrid_store(v, called ? best : tg.fill, best_n, total, state_out, support, covered);
    }
    wave_run_add(hist, key, key >= 0 ? 1ull : 0ull);
    wave_add(hist + K + 1, is_mixed);
  }
  if (wrong) atomicOr(bad, wrong);
}

__global__ __launch_bounds__(64 * REGRID_WAVES) void regrid_wave_kernel(const uint8_t* __restrict__ labels,
                                                                        const RegridPiece* __restrict__ pieces,
                                                                        const RegridAxis* __restrict__ rows,
                                                                        const RegridAxis* __restrict__ cols, RegridTarget tg,
                                                                        uint8_t* __restrict__ state_out, unsigned* __restrict__ support,
                                                                        unsigned* __restrict__ covered,
                                                                        unsigned long long* __restrict__ hist, int* __restrict__ bad) {
  __shared__ unsigned hist_all[REGRID_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, K = tg.K;
  unsigned* const bins = hist_all[wave];
  bins[lane] = 0;
  wave_order();
  int wrong = 0;
  for (long long v = (long long)blockIdx.x * REGRID_WAVES + wave; v < tg.n_t; v += (long long)gridDim.x * REGRID_WAVES) {
    int r, c;
    regrid_cell(v, tg, &r, &c);
    const RegridAxis ax = rows[r], ay = cols[c];
    for (int t = 0; t < tg.npieces; ++t) {
      const RegridPiece pc = pieces[t];
      int i0, i1, j0, j1;
      if (!regrid_clip(pc, ax, ay, &i0, &i1, &j0, &j1)) continue;                    // (the same for the whole wave)
      const uint8_t* const lab = labels + pc.lo;
      const RegridAxis& other = pc.mirror ? ax : ay;
      for (int i = i0; i < i1; ++i) {
        const long long bin_i = (long long)pc.s1 + i;
        const long long same = pc.mirror ? bin_i - pc.s2 : -1;                       // the column of the bin pair (p, p)
        const unsigned wi = pc.mirror ? regrid_weight(ay, bin_i - ay.p0, tg.inner) : regrid_weight(ax, bin_i - ax.p0, tg.inner);
        auto key_of = [&](int s, int j) -> int {
          if (j == same) return -1;
          if (s >= K) {
            wrong = 1;
            return -1;
          }
          return s;
        };
        auto weight_of = [&](int j) -> unsigned { return wi * regrid_weight(other, (long long)pc.s2 + j - other.p0, tg.inner); };
        for (int jb = (pc.diagonal && j0 < i) ? i : j0; jb < j1; jb += REGRID_ROW_W) {       // (i < i1 <= j1 in a diagonal block)
          const LabelRow row = label_row(lab, i, jb, jb + REGRID_ROW_W < j1 ? jb + REGRID_ROW_W : j1, pc.W, pc.diagonal);
          uint32_t word = 0;
          int single = 0;
          load_row(row, lane, &word, &single);
          if (row.nvec > 0) {
            int key[4] = {-1, -1, -1, -1};
            unsigned x[4] = {0, 0, 0, 0};
            if (lane < row.nvec) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int j = row.ja + row.head + 4 * lane + e;
                key[e] = key_of((int)((word >> (8 * e)) & 0xff), j);
                x[e] = weight_of(j);
              }
            }
            wave_quad_add(bins, key, x);
          }
          if (row.nbytes > 0) {
            int key = -1;
            unsigned x = 0;
            if (lane < row.nbytes) {
              const int j = row.ja + row.byte_at(lane);
              key = key_of(single, j);
              x = weight_of(j);
            }
            wave_run_add(bins, key, key >= 0 ? x : 0u);
          }
        }
      }
    }
    wave_order();
    unsigned mine = bins[lane];                        // lane k: the cell's votes for state k (no key is >= K)
    bins[lane] = 0;
    wave_order();
    unsigned total = mine, best_n = mine;
    int best = lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      total += __shfl_xor(total, off, 64);
      const unsigned n = __shfl_xor(best_n, off, 64);
      const int k = __shfl_xor(best, off, 64);
      if (n > best_n || (n == best_n && k < best)) {
        best_n = n;
        best = k;
      }
    }
    if (lane == 0) {
      const bool called = total >= tg.min_cover;
      regrid_store(v, called ? best : tg.fill, best_n, total, state_out, support, covered);
      atomicAdd(hist + (called ? best : K), 1ull);
      if (called && best_n < total) atomicAdd(hist + K + 1, 1ull);
    }
  }
  if (wrong) atomicOr(bad, wrong);
}

// the axis table of n target bins from `start` on
void regrid_axis(int64_t start, int n, int a, int b, std::vector<RegridAxis>* out) {
  out->resize((size_t)n);
  for (int t = 0; t < n; ++t) {
    const int64_t u0 = (start + t) * b, u1 = u0 + b;   // below 2^47
    const int64_t p0 = u0 / a, p1 = (u1 + a - 1) / a;
    const int64_t first_end = (p0 + 1) * a < u1 ? (p0 + 1) * a : u1, last_start = (p1 - 1) * a > u0 ? (p1 - 1) * a : u0;
    (*out)[(size_t)t] = RegridAxis{(long long)p0, (int)(p1 - p0), (int)(first_end - u0), (int)(u1 - last_start), 0};
  }
}

// [lo, hi) and [lo2, hi2) share a bin
inline bool regrid_meet(int64_t lo, int64_t hi, int64_t lo2, int64_t hi2) { return lo < hi2 && lo2 < hi; }

}  // namespace
}  // namespace phmrf

using namespace phmrf;

extern "C" {

int phmrf_regrid_states(const uint8_t* labels_dev, int64_t n_labels, int R, const int64_t* regions_host, int K, int a, int b, int H,
                        int W, int diagonal, int64_t start_bin1, int64_t start_bin2, int64_t min_cover, int fill, uint8_t* state_dev,
                        uint32_t* support_dev_or_null, uint32_t* covered_dev_or_null, int64_t* hist_host, int64_t* mixed_host,
                        void* hip_stream) {
  PHMRF_CHECK(labels_dev && regions_host && state_dev && hist_host && mixed_host, PHMRF_ERR_INVALID,
              "NULL labels, regions, state plane, histogram or mixed count");
  PHMRF_CHECK(n_labels >= 1, PHMRF_ERR_INVALID, "n_labels must be >= 1");
  PHMRF_CHECK(R >= 1, PHMRF_ERR_INVALID, "R must be >= 1");
  PHMRF_CHECK(a >= 1 && b >= 1, PHMRF_ERR_INVALID, "a and b must be >= 1");
  PHMRF_CHECK(fill >= 0 && fill <= 255, PHMRF_ERR_INVALID, "fill must be in 0 .. 255");
  PHMRF_TRY(check_states(K));
  PHMRF_CHECK(R <= REGRID_MAX_REGIONS, PHMRF_ERR_UNSUPPORTED, "R must be <= 64");
  PHMRF_CHECK(a <= REGRID_MAX_RATIO && b <= REGRID_MAX_RATIO, PHMRF_ERR_UNSUPPORTED, "a and b must be <= 2^15");
  PHMRF_CHECK(min_cover >= 1 && min_cover <= (int64_t)b * b, PHMRF_ERR_INVALID, "min_cover must be in 1 .. b^2");
  int64_t n_t = 0;
  PHMRF_TRY(check_region(H, W, diagonal, &n_t));
  PHMRF_CHECK(start_bin1 >= 0 && start_bin2 >= 0, PHMRF_ERR_INVALID, "the target's start bins must be >= 0");
  PHMRF_CHECK(!diagonal || start_bin1 == start_bin2, PHMRF_ERR_INVALID, "a diagonal target has start_bin1 == start_bin2");
  PHMRF_CHECK(!coord_out(start_bin1) && !coord_out(start_bin2), PHMRF_ERR_UNSUPPORTED, "the target's start bins must be below 2^30");
  PHMRF_TRY(check_nodes(n_t, "the target region must have fewer than 2^31 - 64 nodes"));
  struct Source {
    int64_t lo, s1, s2;
    int H, W, diagonal;
  };
  std::vector<Source> src((size_t)R);
  for (int r = 0; r < R; ++r) {
    const int64_t* row = regions_host + 6 * (size_t)r;
    PHMRF_CHECK(row[1] >= 1 && row[2] >= 1, PHMRF_ERR_INVALID, "H and W must be >= 1");
    PHMRF_CHECK(row[1] < ((int64_t)1 << 31) && row[2] < ((int64_t)1 << 31), PHMRF_ERR_UNSUPPORTED, "H and W must be below 2^31");
    PHMRF_CHECK(row[5] == 0 || row[5] == 1, PHMRF_ERR_INVALID, "diagonal must be 0 or 1");
    int64_t n = 0;
    PHMRF_TRY(check_region((int)row[1], (int)row[2], (int)row[5], &n));
    PHMRF_TRY(check_nodes(n));
    PHMRF_CHECK(row[0] >= 0 && row[0] + n <= n_labels, PHMRF_ERR_INVALID, "a region's nodes must lie inside the labels");
    PHMRF_CHECK(row[3] >= 0 && row[4] >= 0, PHMRF_ERR_INVALID, "a region's start bins must be >= 0");
    PHMRF_CHECK(!coord_out(row[3]) && !coord_out(row[4]), PHMRF_ERR_UNSUPPORTED, "a region's start bins must be below 2^30");
    PHMRF_CHECK(!row[5] || row[3] == row[4], PHMRF_ERR_INVALID,
                "source region " + std::to_string(r) + " is diagonal with start_bin1 != start_bin2");
    src[(size_t)r] = Source{row[0], row[3], row[4], (int)row[1], (int)row[2], (int)row[5]};
  }
  // no two source regions may hold one cell of the full matrix, directly or through a mirror
  for (int r = 0; r < R; ++r) {
    const Source& p = src[(size_t)r];
    PHMRF_CHECK(p.diagonal || !regrid_meet(p.s1, p.s1 + p.H, p.s2, p.s2 + p.W), PHMRF_ERR_INVALID,
                "source region " + std::to_string(r) + " overlaps its own mirror image: its rows and columns share a bin");
    for (int s = r + 1; s < R; ++s) {
      const Source& q = src[(size_t)s];
      const bool direct = regrid_meet(p.s1, p.s1 + p.H, q.s1, q.s1 + q.H) && regrid_meet(p.s2, p.s2 + p.W, q.s2, q.s2 + q.W);
      const bool mirrored = regrid_meet(p.s1, p.s1 + p.H, q.s2, q.s2 + q.W) && regrid_meet(p.s2, p.s2 + p.W, q.s1, q.s1 + q.H);
      PHMRF_CHECK(!direct && !mirrored, PHMRF_ERR_INVALID,
                  "source regions " + std::to_string(r) + " and " + std::to_string(s) + " overlap" +
                      (direct ? "" : " through the mirror image"));
    }
  }
  std::vector<RegridAxis> rows, cols;
  regrid_axis(start_bin1, H, a, b, &rows);
  regrid_axis(start_bin2, W, a, b, &cols);
  const long long P0 = rows.front().p0, P1 = rows.back().p0 + rows.back().n, Q0 = cols.front().p0, Q1 = cols.back().p0 + cols.back().n;
  std::vector<RegridPiece> pieces;
  for (int r = 0; r < R; ++r) {
    const Source& p = src[(size_t)r];
    for (int mirror = 0; mirror < 2; ++mirror) {
      RegridPiece pc{(long long)p.lo, p.W, p.diagonal, (int)p.s1, (int)p.s2, 0, 0, 0, 0, mirror, 0};
      if (clip_rect(p.H, p.W, p.diagonal, (mirror ? Q0 : P0) - p.s1, (mirror ? Q1 : P1) - p.s1, (mirror ? P0 : Q0) - p.s2,
                    (mirror ? P1 : Q1) - p.s2, &pc.i0, &pc.i1, &pc.j0, &pc.j1))
        pieces.push_back(pc);
    }
  }
  const int64_t nmax = 1 + ((int64_t)b - 1 + a - 1) / a;      // the most source bins a target bin meets
  const bool small = nmax * nmax <= REGRID_SMALL_AREA;
  const RegridTarget tg{H, W, diagonal, K, a, (unsigned)min_cover, fill, (int)pieces.size(), (long long)n_t};

  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  Buffers buf;
  FlaggedTable tab(st);                                // hist [K + 1] | mixed
  RegridPiece* pieces_dev;
  RegridAxis *rows_dev, *cols_dev;
  uint8_t* state_tmp;
  unsigned *support_tmp = nullptr, *covered_tmp = nullptr;
  PHMRF_TRY(tab.make(&buf, (size_t)K + 2));
  PHMRF_TRY(buf.get(&pieces_dev, pieces.size()));
  PHMRF_TRY(buf.get(&rows_dev, rows.size()));
  PHMRF_TRY(buf.get(&cols_dev, cols.size()));
  PHMRF_TRY(buf.get(&state_tmp, (size_t)n_t));
  if (support_dev_or_null) PHMRF_TRY(buf.get(&support_tmp, (size_t)n_t));
  if (covered_dev_or_null) PHMRF_TRY(buf.get(&covered_tmp, (size_t)n_t));
  if (!pieces.empty())
    PHMRF_HIP(hipMemcpyAsync(pieces_dev, pieces.data(), pieces.size() * sizeof(RegridPiece), hipMemcpyHostToDevice, st));
  PHMRF_HIP(hipMemcpyAsync(rows_dev, rows.data(), rows.size() * sizeof(RegridAxis), hipMemcpyHostToDevice, st));
  PHMRF_HIP(hipMemcpyAsync(cols_dev, cols.data(), cols.size() * sizeof(RegridAxis), hipMemcpyHostToDevice, st));
  if (small) {
    const int64_t ntiles = (n_t + REGRID_LANES - 1) / REGRID_LANES;
    hipLaunchKernelGGL(regrid_lane_kernel, dim3(grid_of(ntiles, 1, REGRID_GRID_CAP)), dim3(REGRID_LANES),
                       (size_t)K * REGRID_LANES * sizeof(unsigned), st, labels_dev, pieces_dev, rows_dev, cols_dev, tg, ntiles,
                       state_tmp, support_tmp, covered_tmp, tab.words(), tab.flag());
  } else {
    hipLaunchKernelGGL(regrid_wave_kernel, dim3(grid_of(n_t, REGRID_WAVES, REGRID_WAVE_GRID_CAP)), dim3(64 * REGRID_WAVES), 0, st,
                       labels_dev, pieces_dev, rows_dev, cols_dev, tg, state_tmp, support_tmp, covered_tmp, tab.words(), tab.flag());
  }
  PHMRF_HIP(hipGetLastError());
  int bad = 0;
  PHMRF_TRY(tab.read_flag(&bad));
  PHMRF_CHECK(!bad, PHMRF_ERR_INVALID, "a label inside a read cell is >= K");
  PHMRF_HIP(hipMemcpyAsync(state_dev, state_tmp, (size_t)n_t, hipMemcpyDeviceToDevice, st));
  if (support_dev_or_null)
    PHMRF_HIP(hipMemcpyAsync(support_dev_or_null, support_tmp, (size_t)n_t * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
  if (covered_dev_or_null)
    PHMRF_HIP(hipMemcpyAsync(covered_dev_or_null, covered_tmp, (size_t)n_t * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
  std::vector<int64_t> counts((size_t)K + 2);
  PHMRF_TRY(tab.copy(0, (size_t)K + 2, counts.data()));
  PHMRF_TRY(tab.wait());
  for (int k = 0; k <= K; ++k) hist_host[k] = counts[(size_t)k];
  *mixed_host = counts[(size_t)K + 1];
  return PHMRF_OK;
}

}  // extern "C"
