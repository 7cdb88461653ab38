"""A state map resampled onto another map's grid: a 10 kb fit against a 50 kb fit of the same
chromosomes, a segmentation whose synteny blocks were split differently, a map made elsewhere on another binning.  The result
is a state map like any other, so --compare, --consensus and every other mode read it.

The source has bins of rs bp and the target bins of rd bp; u = gcd(rs, rd), a = rs / u, b = rd / u (both at most 2^15).  Source
bin p covers the units [p a, (p + 1) a), target bin x the units [x b, (x + 1) b) and
    ov(x, p) = max(0, min((x + 1) b, (p + 1) a) - max(x b, p a))
(`overlap`, the one place the rule is written in Python).  For a target bin pair (x, y) of one chromosome, over the stored
nodes (p, q) = (start_bin1 + i, start_bin2 + j) of all source regions of that chromosome in state k,
    votes[x][y][k] = sum of ov(x, p) ov(y, q) + [p != q] ov(x, q) ov(y, p):
the symmetric chromosome matrix read through all its regions at once, exactly across region seams and through mirror halves;
a target cell on the diagonal counts off-diagonal source cells twice, as --render does.  covered = sum_k votes <= b^2,
support = max_k votes, the called state is the lowest k at the maximum, and a cell is CALLED when covered >= min_cover,
else it takes `fill` = K, "uncovered" (core_vec's convention in --consensus).  The source regions must not overlap on the full
matrix (`check_disjoint`): covered / b^2 is a true share.

`regrid_states(...)` computes on the GPU, one phmrf_regrid_states call (csrc/regrid.hip) per target region with the source
regions of that region's chromosome; `derive_len_vec(...)` gives the source's own regions on the new binning; `save_mat` and
`summary_lines` write the result, `regrid_files(...)` is the command line's --regrid SRC.mat.

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np

from .maps import MAX_STATES, check_K, check_len_vec, check_resolution, check_state_vec, device, load_map, stem

LANES = 128                      # csrc/regrid.hip REGRID_LANES: target cells of a tile = lanes of a workgroup of the lane kernel
GRID_CAP = 4096                  # csrc/regrid.hip REGRID_GRID_CAP: workgroups of the lane kernel
SMALL_AREA = 256                 # csrc/regrid.hip REGRID_SMALL_AREA: when the largest source rectangle of a target cell,
#                                  max_bins(a, b)^2 source cells, is above this, a wave walks a target cell, not a lane
WAVES = 4                        # csrc/regrid.hip REGRID_WAVES: waves of a workgroup of the wave kernel
WAVE_GRID_CAP = 2048             # csrc/regrid.hip REGRID_WAVE_GRID_CAP: workgroups of the wave kernel
ROW_W = 256                      # csrc/regrid.hip REGRID_ROW_W: columns of a storage row the wave kernel takes at a time
MAX_REGIONS = 64                 # csrc/regrid.hip REGRID_MAX_REGIONS: source regions of one chromosome
MAX_RATIO = 1 << 15              # csrc/regrid.hip REGRID_MAX_RATIO: a, b <= 2^15
FIELDS = ("state_vec", "state_vec_smooth")


def ratio(src_resolution, dst_resolution):
    """-> (a, b): the units of a source bin and of a target bin, the bin sizes over their greatest common divisor"""
    rs, rd = check_resolution(src_resolution), check_resolution(dst_resolution)
    u = math.gcd(rs, rd)
    a, b = rs // u, rd // u
    if a > MAX_RATIO or b > MAX_RATIO:
        raise ValueError("%d bp and %d bp are %d : %d in lowest terms: both must be at most %d" % (rs, rd, a, b, MAX_RATIO))
    return a, b


def overlap(x, p, a, b):
    """ov(x, p): the units target bin x = [x b, (x + 1) b) and source bin p = [p a, (p + 1) a) share.  Host only."""
    x, p, a, b = int(x), int(p), int(a), int(b)
    return max(0, min((x + 1) * b, (p + 1) * a) - max(x * b, p * a))


def max_bins(a, b):
    """the most source bins one target bin meets on an axis: 1 + ceil((b - 1) / a)"""
    return 1 + (int(b) - 1 + int(a) - 1) // int(a)


def is_small(a, b):
    """whether a call at (a, b) goes through the kernel of a lane per target cell: max_bins(a, b)^2 <= SMALL_AREA"""
    return max_bins(a, b) ** 2 <= SMALL_AREA


def min_cover_of(cover, b):
    """-> min_cover = max(1, ceil(cover b^2 / 100)) in Python integers; cover in percent, 0 .. 100 (0: any coverage)"""
    c = Fraction(str(cover)) if not isinstance(cover, (int, np.integer)) else Fraction(int(cover))
    if c < 0 or c > 100:
        raise ValueError("cover must be in 0 .. 100 percent")
    num, den = c.numerator * int(b) * int(b), c.denominator * 100
    return max(1, -(-num // den))


def _meet(lo, hi, lo2, hi2):
    return lo < hi2 and lo2 < hi


def check_disjoint(len_vec):
    """ValueError when two regions of one chromosome hold one cell of the full matrix, directly or through a mirror image: an
    off-diagonal region whose row and column ranges share a bin overlaps its own, a diagonal region must have start_bin1 ==
    start_bin2.  The message names the regions by their row in len_vec.  Host only."""
    L = np.asarray(len_vec)
    box = [(int(r[5]), int(r[5]) + int(r[3]), int(r[6]), int(r[6]) + int(r[4]), int(r[8]), int(r[9])) for r in L]
    for r, (r0, r1, c0, c1, diag, chrom) in enumerate(box):
        if diag and r0 != c0:
            raise ValueError("len_vec row %d: a diagonal region with start_bin1 != start_bin2" % r)
        if not diag and _meet(r0, r1, c0, c1):
            raise ValueError("len_vec row %d overlaps its own mirror image: its rows and columns share a bin" % r)
        for s in range(r + 1, len(box)):
            q0, q1, d0, d1, _, chrom_s = box[s]
            if chrom_s != chrom:
                continue
            if _meet(r0, r1, q0, q1) and _meet(c0, c1, d0, d1):
                raise ValueError("len_vec rows %d and %d overlap" % (r, s))
            if _meet(r0, r1, d0, d1) and _meet(c0, c1, q0, q1):
                raise ValueError("len_vec rows %d and %d overlap through the mirror image" % (r, s))


def derive_len_vec(len_vec, src_resolution, dst_resolution):
    """-> int64 [R, 10]: the source's own regions on the new binning.  Rows become [floor(s1 a / b), ceil((s1 + H) a / b)),
    columns likewise; a diagonal region stays diagonal; region_id and chrom are kept; n, start and stop are recomputed back
    to back.  Host only."""
    a, b = ratio(src_resolution, dst_resolution)
    L = _regions_of(len_vec)
    out, at = np.zeros((L.shape[0], 10), dtype=np.int64), 0
    for r, row in enumerate(L):
        H, W, s1, s2, rid, diag, chrom = (int(row[x]) for x in (3, 4, 5, 6, 7, 8, 9))
        x0, x1 = (s1 * a) // b, -(-((s1 + H) * a) // b)
        y0, y1 = (s2 * a) // b, -(-((s2 + W) * a) // b)
        h, w = x1 - x0, y1 - y0
        n = h * (h + 1) // 2 if diag else h * w
        out[r] = [n, at, at + n, h, w, x0, y0, rid, diag, chrom]
        at += n
    return out


def _regions_of(len_vec):
    """a len_vec checked row by row without its state_vec: every slice holds the nodes its shape says"""
    return check_len_vec(len_vec, 1 << 62)


def _check_target(dst_len_vec):
    D = _regions_of(dst_len_vec)
    for r, row in enumerate(D):
        if int(row[8]) == 1 and int(row[5]) != int(row[6]):
            raise ValueError("dst_len_vec row %d: a diagonal region with start_bin1 != start_bin2" % r)
    return D


def regrid_states(state_vec, len_vec, src_resolution, dst_len_vec, dst_resolution, K=None, cover=50):
    """The source map (state_vec, len_vec) at src_resolution bp on the regions of dst_len_vec at dst_resolution bp -> dict:
      state_vec uint8 [n]            the called state per stored target cell, `fill` where covered < min_cover
      support, covered uint32 [n]    max_k votes and sum_k votes, of called and uncalled cells alike
      conf float32 [n]               support / covered, 0 where uncalled: the vote share
      cover float32 [n]              covered / b^2
      hist_region int64 [R_t, K + 1] the cells of a target region called k; column K: the uncalled ones
      mixed_region int64 [R_t]       the called cells with support < covered
      K, fill, a, b, min_cover
    n is the largest stop of dst_len_vec.  The map is uploaded once; every target region gets one phmrf_regrid_states call
    with the source regions of its chromosome, a chromosome the source lacks gives all `fill`.  K: the largest state + 1 by
    default; fill = K; cover in percent, min_cover = max(1, ceil(cover b^2 / 100)).  ValueError for overlapping source regions
    (check_disjoint) and, at K = 64, for any uncalled cell: no u8 state is left to mark it.  A state >= K inside a read
    cell is an error (RuntimeError).  RuntimeError without a GPU."""
    from . import _lib
    import torch
    s = check_state_vec(state_vec)
    L = check_len_vec(len_vec, s.shape[0])
    check_disjoint(L)
    D = _check_target(dst_len_vec)
    a, b = ratio(src_resolution, dst_resolution)
    K = check_K(s, K)
    fill = K
    min_cover = min_cover_of(cover, b)
    lib, dev, stream = device()
    n = int(D[:, 2].max())
    Rt = D.shape[0]
    state_t = torch.full((n,), fill, dtype=torch.uint8, device=dev)
    support_t = torch.zeros((n,), dtype=torch.int32, device=dev)
    covered_t = torch.zeros((n,), dtype=torch.int32, device=dev)
    hist_region = np.zeros((Rt, K + 1), dtype=np.int64)
    mixed_region = np.zeros(Rt, dtype=np.int64)
    s_t = torch.from_numpy(s.astype(np.uint8)).to(dev) if s.size else None
    for t, row in enumerate(D):
        n_t, lo, H, W, t1, t2, diag, chrom = (int(row[x]) for x in (0, 1, 3, 4, 5, 6, 8, 9))
        rows = L[L[:, 9] == chrom]
        if not rows.shape[0] or s_t is None:
            hist_region[t, K] = n_t
            continue
        if rows.shape[0] > MAX_REGIONS:
            raise ValueError("chromosome %d has %d regions, above %d" % (chrom, rows.shape[0], MAX_REGIONS))
        regs = np.ascontiguousarray(rows[:, [1, 3, 4, 5, 6, 8]], dtype=np.int64)
        mixed = ctypes.c_int64(0)
        _lib.check(lib.phmrf_regrid_states(ctypes.c_void_p(s_t.data_ptr()), s.shape[0], regs.shape[0], _lib.ptr_i64(regs), K, a, b, H, W,
                                           diag, t1, t2, min_cover, fill, ctypes.c_void_p(state_t.data_ptr() + lo),
                                           ctypes.c_void_p(support_t.data_ptr() + 4 * lo), ctypes.c_void_p(covered_t.data_ptr() + 4 * lo),
                                           _lib.ptr_i64(hist_region[t]), ctypes.byref(mixed), stream))
        mixed_region[t] = mixed.value
    check_uncalled(K, int(hist_region[:, K].sum()))
    state = state_t.cpu().numpy()
    support = support_t.cpu().numpy().view(np.uint32)
    covered = covered_t.cpu().numpy().view(np.uint32)
    return dict(derived_planes(state, support, covered, fill, b), hist_region=hist_region, mixed_region=mixed_region, K=np.int64(K),
                fill=np.int64(fill), a=np.int64(a), b=np.int64(b), min_cover=np.int64(min_cover))


def check_uncalled(K, uncalled):
    """ValueError at K = 64 with uncalled cells: fill = K = 64 is no state a map can hold.  Host only."""
    if int(K) == MAX_STATES and int(uncalled) > 0:
        raise ValueError("%d cells are uncalled and K = %d leaves no state to mark them: lower cover, or pass a target that the "
                         "source covers" % (int(uncalled), MAX_STATES))


def derived_planes(state, support, covered, fill, b):
    """-> dict of state_vec, support, covered and the planes the host derives from these integers: conf float32 = support /
    covered (0 where the state is `fill`) and cover float32 = covered / b^2.  Host only."""
    state, support, covered = np.asarray(state), np.asarray(support), np.asarray(covered)
    called = state != fill
    conf = np.zeros(state.shape[0], dtype=np.float32)
    conf[called] = (support[called].astype(np.float64) / covered[called].astype(np.float64)).astype(np.float32)
    cover = (covered.astype(np.float64) / float(int(b) * int(b))).astype(np.float32)
    return dict(state_vec=state, support=support, covered=covered, conf=conf, cover=cover)


# ---- reading and writing --------------------------------------------------------------------------------------------------
def summary_lines(result, dst_len_vec):
    """-> the lines of regrid_*.txt, header first: per target region its id, chromosome and start bins, the cells, the called,
    uncalled and unanimous (called with support == covered) counts, the mean cover, then the K + 1 counts of hist_region"""
    D, K = np.asarray(dst_len_vec), int(result["K"])
    lines = ["\t".join(["#region", "chrom", "start_bin1", "start_bin2", "cells", "called", "uncalled", "unanimous", "mean_cover"] +
                       ["state%d" % (k + 1) for k in range(K)] + ["uncovered"]) + "\n"]
    for t, row in enumerate(D):
        hist = np.asarray(result["hist_region"])[t]
        cells, uncalled = int(hist.sum()), int(hist[K])
        cover = np.asarray(result["cover"])[int(row[1]):int(row[2])]
        mean = float(cover.astype(np.float64).mean()) if cover.size else 0.0
        f = ["%d" % row[7], "%d" % row[9], "%d" % row[5], "%d" % row[6], "%d" % cells, "%d" % (cells - uncalled), "%d" % uncalled,
             "%d" % (cells - uncalled - int(np.asarray(result["mixed_region"])[t])), "%.6f" % mean]
        lines.append("\t".join(f + ["%d" % x for x in hist]) + "\n")
    return lines


def save_mat(path, result, dst_len_vec, src_len_vec, src_resolution, dst_resolution, field="state_vec", cover=50, source=""):
    """write regrid_*.mat: the result as a state map (state_vec, len_vec, conf), its planes and counts, uncovered_state (K, or
    -1 when every cell is called), src_len_vec and the settings.  Host only."""
    import scipy.io
    out = dict((k, v) for k, v in result.items() if k != "fill")
    uncalled = int(np.asarray(result["hist_region"])[:, int(result["K"])].sum())
    out.update(len_vec=np.asarray(dst_len_vec), src_len_vec=np.asarray(src_len_vec),
               uncovered_state=np.int64(int(result["fill"]) if uncalled else -1), resolution=np.int64(int(dst_resolution)),
               regrid_from=np.int64(int(src_resolution)), regrid_field=field, regrid_cover=float(cover), regrid_source=str(source))
    scipy.io.savemat(path, out)


def regrid_files(path, output_path, src_resolution, dst_resolution, like="", field="state_vec", cover=50):
    """The command line's --regrid: resample the `field` of one estimate_ou_*.mat / segment_*.mat / smooth_*.mat from
    src_resolution bp onto dst_resolution bp, on the regions of the .mat `like` (its len_vec verbatim, with all its columns)
    or else on derive_len_vec's.  Writes under output_path regrid_<stem>_<dst_resolution>.mat (save_mat) and .txt
    (summary_lines).  -> the .mat"""
    import scipy.io
    if field not in FIELDS:
        raise ValueError("field must be state_vec or state_vec_smooth, not %r" % (field,))
    rs, rd = check_resolution(src_resolution), check_resolution(dst_resolution)
    s, L, _ = load_map(path, field)
    if like:
        d = scipy.io.loadmat(like)
        if "len_vec" not in d:
            raise ValueError("%s holds no len_vec" % like)
        D = _regions_of(d["len_vec"])
    else:
        D = derive_len_vec(L, rs, rd)
    res = regrid_states(s, L, rs, D, rd, cover=cover)
    os.makedirs(output_path, exist_ok=True)
    name = "regrid_%s_%d" % (stem(path), rd)
    out = os.path.join(output_path, name + ".mat")
    save_mat(out, res, D, L, rs, rd, field=field, cover=cover, source=os.path.basename(path))
    with open(os.path.join(output_path, name + ".txt"), "wb") as fh:
        fh.write("".join(summary_lines(res, D)).encode())
    return out
