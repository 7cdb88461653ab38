"""The state composition of listed interval pairs: which state does this loop, this TAD, this TAD pair,
this enhancer-promoter pair hold, how pure is it, and how does it compare with the same rectangle moved along the diagonal.

A query is (chrom, a0, a1, b0, b1): two half-open bin intervals A = [a0, a1) and B = [b0, b1) of one chromosome, in either
order; they may overlap or be equal.  Its bin pairs are the unordered pairs {i, j} with (i in A and j in B) or (i in B and
j in A) -- {i, i} belongs when i is in both --, |A||B| - m (m - 1) / 2 of them with m = |A and B| (`n_pairs`); A = B of n bins
gives the n (n + 1) / 2 bin pairs inside a TAD.  A stored node (i, j) of a region stands for the bin pair
{start_bin1 + i, start_bin2 + j}, in a diagonal region (i <= j) and in an off-diagonal one alike, so counts[q][k] = the
stored nodes, over all regions of the chromosome, whose bin pair belongs to query q and whose state is k: every stored node
once, and covered[q] = sum_k counts[q][k] <= pairs[q] with equality when the regions cover the query.

With prim(region, I x J) the histogram of the region's stored nodes with the row bin in I and the column bin in J, per region
    counts = prim(A x B) + prim(B x A) - prim((A and B) x (A and B))
(`rectangles`: at most three signed rectangles per query and region, one when A = B), and prim is what the GPU computes
(phmrf_rect_states, csrc/query.hip).  `state_query(...)` runs it region by region and sums; `read_intervals(...)` reads a BED
file into queries with A = B, `read_pairs(...)` a BEDPE file, `with_controls(...)` gives the queries shifted ALONG the
diagonal (the same genomic distance: the project's rule for an expectation), `query_files(...)` is the command line's --query.

THE BIN RULE: an interval [start, stop) in bp becomes the bins it OVERLAPS, a0 = start // res, a1 = max(a0 + 1,
ceil(stop / res)): a 5 kb loop anchor at 50 kb still has its bin.  This differs on purpose from --pileup, which takes the ONE
bin of the interval's midpoint, and from --enrich, which gives a bin to the class that holds its midpoint.

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

from .intervals import (check_shift, held_chrom, held_chroms, interval_lines, log2_ratio, overlap_bins, pile_summary, shift_along_diagonal,
                        summary_fields)
from .maps import CONF_ONE, check_K, check_len_vec, check_resolution, check_state_vec, conf_array, device, load_map, regions, stem

TILE_H = 16                      # csrc/query.hip RECT_TILE_H: storage rows of an item, the piece of a rectangle one wave takes
TILE_W = 256                     # csrc/query.hip RECT_TILE_W: storage columns of an item
VEC_MIN = 32                     # csrc/query.hip RECT_VEC_MIN: an item at least this wide is read in aligned 4-byte words
WAVES = 4                        # csrc/query.hip RECT_WAVES: waves of a workgroup
GRID_CAP = 2048                  # csrc/query.hip RECT_GRID_CAP: workgroups
BATCH = 1 << 20                  # csrc/query.hip RECT_BATCH: items uploaded and launched together
COORD_LIMIT = 1 << 30            # csrc/interval_lists.h COORD_LIMIT: |c| of a rectangle's coordinate stays below it


def _check_queries(queries):
    """-> int64 [N, 5]: chrom, a0, a1, b0, b1"""
    q = np.asarray(queries)
    if q.size == 0:
        return np.zeros((0, 5), dtype=np.int64)
    if q.ndim != 2 or q.shape[1] != 5 or q.dtype.kind not in "iu":
        raise ValueError("queries must be an integer array of rows chrom, a0, a1, b0, b1 (got %s %s)" % (q.dtype, q.shape))
    q = q.astype(np.int64)
    if np.any(q[:, 2] < q[:, 1]) or np.any(q[:, 4] < q[:, 3]):
        raise ValueError("a query's intervals are half-open [a0, a1) and [b0, b1): a1 >= a0 and b1 >= b0")
    if np.abs(q[:, 1:]).max() >= COORD_LIMIT:
        raise ValueError("a query's bins must stay below 2^30")
    return q


def n_pairs(queries):
    """-> int64 [N]: the bin pairs of every query, |A||B| - m (m - 1) / 2 with m = |A and B|.  Host only."""
    q = _check_queries(queries)
    m = np.maximum(0, np.minimum(q[:, 2], q[:, 4]) - np.maximum(q[:, 1], q[:, 3]))
    return (q[:, 2] - q[:, 1]) * (q[:, 4] - q[:, 3]) - m * (m - 1) // 2


def with_controls(queries, shift_bins):
    """-> (controls int64 [M, 5], owner int64 [M]): for every query the two queries shifted by -shift and by +shift bins
    ALONG the diagonal -- both intervals move together, so every bin pair keeps its genomic distance --, the one before its
    query first; owner[c] is the index of control c's query.  A control with a negative bin is dropped.  Host only."""
    q = _check_queries(queries)
    ctl, keep = shift_along_diagonal(q, ((1, 2), (3, 4)), shift_bins)
    return ctl[keep], np.repeat(np.arange(q.shape[0], dtype=np.int64), 2)[keep]


def region_rectangles(queries, row):
    """What one region (a row of len_vec) is given of checked queries [N, 5] -> (rect int32 [R, 4] of rows i0, i1, j0, j1 local
    to the region and clipped to it, slot int32 [R]: the query's index, minus u8 [R]): A x B, and for A != B also B x A and,
    subtracted, (A and B)^2; without the rectangles that are empty after clipping and, in a diagonal region, those wholly
    below the diagonal (i0 >= j1).  Host only."""
    H, W, s1, s2, diag = (int(row[x]) for x in (3, 4, 5, 6, 8))
    idx = np.flatnonzero(queries[:, 0] == row[9])
    a0, a1, b0, b1 = (queries[idx, c] for c in (1, 2, 3, 4))
    c0, c1 = np.maximum(a0, b0), np.minimum(a1, b1)
    differ = (a0 != b0) | (a1 != b1)                        # A == B: the second and the third rectangle cancel
    # rows: the three rectangles of every query as (row interval, column interval, sign, is it submitted)
    parts = ((a0, a1, b0, b1, 0, np.ones(idx.shape, dtype=bool)), (b0, b1, a0, a1, 0, differ), (c0, c1, c0, c1, 1, differ & (c1 > c0)))
    rect = np.stack([np.stack([np.clip(r0 - s1, 0, H), np.clip(r1 - s1, 0, H), np.clip(k0 - s2, 0, W), np.clip(k1 - s2, 0, W)], axis=1)
                     for r0, r1, k0, k1, _, _ in parts], axis=1).reshape(-1, 4)
    slot = np.repeat(idx, 3)
    minus = np.tile(np.array([p[4] for p in parts], dtype=np.uint8), idx.shape[0])
    keep = np.stack([p[5] for p in parts], axis=1).reshape(-1) & (rect[:, 1] > rect[:, 0]) & (rect[:, 3] > rect[:, 2])
    if diag:
        keep &= rect[:, 0] < rect[:, 3]
    return rect[keep].astype(np.int32), slot[keep].astype(np.int32), minus[keep]


def rectangles(queries, len_vec):
    """-> per region of len_vec its (rect, slot, minus) of region_rectangles: the reduction of the queries' bin pairs to signed
    rectangles of stored nodes, exact across the regions and the mirror halves of a chromosome.  Host only."""
    q = _check_queries(queries)
    return [region_rectangles(q, row) for row in np.asarray(len_vec)]


def region_states(lib, stream, labels_ptr, conf_ptr, H, W, diag, K, rect, slot, minus):
    """One phmrf_rect_states call for the rectangles of one region -> (rows int64 [U]: the slots that occur, ascending, counts
    int64 [U, K], conf_sum int64 [U] or None without conf_ptr).  The call's tables hold a row per slot that occurs, not per
    query: a region of a genome-wide list is not charged for the other chromosomes' queries."""
    from . import _lib
    rows, local = np.unique(slot, return_inverse=True)
    rect, local = np.ascontiguousarray(rect, dtype=np.int32), np.ascontiguousarray(local, dtype=np.int32)
    minus = np.ascontiguousarray(minus, dtype=np.uint8)
    counts = np.zeros((rows.shape[0], K), dtype=np.int64)
    conf_sum = None if conf_ptr is None else np.zeros(rows.shape[0], dtype=np.int64)
    _lib.check(lib.phmrf_rect_states(labels_ptr, conf_ptr, H, W, diag, K, rect.shape[0], _lib.ptr_i32(rect), _lib.ptr_i32(local),
                                     minus.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), rows.shape[0], _lib.ptr_i64(counts),
                                     None if conf_ptr is None else _lib.ptr_i64(conf_sum), stream))
    return rows.astype(np.int64), counts, conf_sum


def state_query(state_vec, len_vec, queries, K=None, conf=None):
    """queries int64 [Q, 5] of rows chrom, a0, a1, b0, b1 in chromosome bins -> dict:
      counts int64 [Q, K]       the stored nodes, over all regions, whose bin pair belongs to query q and whose state is k
      conf_sum int64 [Q]        the sum of (uint64)(conf 2^24) over those nodes (maps.CONF_ONE), None without conf
      covered int64 [Q]         sum_k counts[q][k]
      pairs int64 [Q]           n_pairs: covered <= pairs, equal when the regions cover the query
      rects_region int64 [R]    the rectangles submitted to each region
      K
    The map, and conf (float32 per node, finite in [0, 1]) when given, are uploaded once; every region that has a rectangle
    gets one phmrf_rect_states call (region_states) and the calls' tables are summed.  K: the largest state + 1 by default; a state >= K inside
    a query is an error (RuntimeError), outside every query it is not looked at.  RuntimeError without a GPU."""
    import torch
    s = check_state_vec(state_vec)
    L = check_len_vec(len_vec, s.shape[0])
    q = _check_queries(queries)
    K = check_K(s, K)
    Q = q.shape[0]
    c = None if conf is None else conf_array(conf, s.shape[0], "conf")
    counts = np.zeros((Q, K), dtype=np.int64)
    conf_sum = None if c is None else np.zeros(Q, dtype=np.int64)
    rects_region = np.zeros(L.shape[0], dtype=np.int64)
    lib, dev, stream = device()
    s_t = torch.from_numpy(s.astype(np.uint8)).to(dev)
    c_t = None if c is None else torch.from_numpy(c).to(dev)
    for r, lo, hi, H, W, diag, _ in regions(L):
        rect, slot, minus = region_rectangles(q, L[r])
        if not rect.shape[0]:
            continue
        rects_region[r] = rect.shape[0]
        rows, part, part_conf = region_states(lib, stream, ctypes.c_void_p(s_t[lo:hi].data_ptr()),
                                              None if c_t is None else ctypes.c_void_p(c_t[lo:hi].data_ptr()), H, W, diag, K, rect, slot, minus)
        counts[rows] += part
        if c is not None:
            conf_sum[rows] += part_conf
    return dict(counts=counts, conf_sum=conf_sum, covered=counts.sum(axis=1), pairs=n_pairs(q), rects_region=rects_region,
                K=np.int64(K))


# ---- the interval files -----------------------------------------------------------------------------------------------------
def _read(rows, names, lines, skipped):
    return dict(queries=np.array(rows, dtype=np.int64).reshape(-1, 5), names=names, lines=lines, skipped_lines=skipped)


def read_intervals(path, len_vec, resolution):
    """A BED file `chrom start stop [name]` (tabs or spaces; lines that start with # and blank lines are skipped) -> dict:
      queries int64 [N, 5]   chrom, a0, a1, a0, a1: every line a query with A = B, the bin pairs inside the interval
      names                  one per query, `.` for a line without one
      lines                  one per query: (chrom as written, start, stop, start, stop) in bp
      skipped_lines          the lines of chromosomes len_vec does not hold
    The interval becomes the bins it OVERLAPS (the module's bin rule, not --pileup's midpoint bin): a0 = start // resolution,
    a1 = max(a0 + 1, ceil(stop / resolution)).  chrom is chr<N> or <N>, N the integer in len_vec's column 9.  ValueError for a
    malformed line, a negative coordinate and stop < start.  Host only."""
    res, held = check_resolution(resolution), held_chroms(len_vec)
    rows, names, lines, skipped = [], [], [], 0
    for _, _, chroms, ((start, stop),), rest in interval_lines(path, 1, "chrom start stop [name]", True):
        c = held_chrom(chroms, held)
        if c is None:
            skipped += 1
            continue
        rows.append([c] + 2 * list(overlap_bins(start, stop, res)))
        names.append(rest[0] if rest else ".")
        lines.append((chroms[0], start, stop, start, stop))
    return _read(rows, names, lines, skipped)


def read_pairs(path, len_vec, resolution):
    """A BEDPE file `chrom1 start1 stop1 chrom2 start2 stop2 [name]` -> read_intervals' dict with the queries chrom, a0, a1,
    b0, b1: A the bins the first interval overlaps, B the second's, in the file's order.  A line whose two ends are not on one
    chromosome of len_vec is skipped and counted.  Host only."""
    res, held = check_resolution(resolution), held_chroms(len_vec)
    rows, names, lines, skipped = [], [], [], 0
    for _, _, chroms, spans, rest in interval_lines(path, 2, "chrom1 start1 stop1 chrom2 start2 stop2 [name]", True):
        c = held_chrom(chroms, held)
        if c is None:
            skipped += 1
            continue
        rows.append([c] + [x for start, stop in spans for x in overlap_bins(start, stop, res)])
        names.append(rest[0] if rest else ".")
        lines.append((chroms[0], *spans[0], *spans[1]))
    return _read(rows, names, lines, skipped)


# ---- reading and writing a table --------------------------------------------------------------------------------------------
def mean_conf(conf_sum, covered):
    """-> float64: conf_sum / (covered 2^24), NaN where covered is 0.  Host only."""
    cs, cov = np.asarray(conf_sum, dtype=np.float64), np.asarray(covered, dtype=np.float64)
    return np.divide(cs, cov * CONF_ONE, out=np.full(cs.shape, np.nan), where=cov > 0)


def control_counts(counts, owner, Q):
    """counts int64 [M, K] of with_controls' M controls -> int64 [Q, K]: summed per owning query.  Host only."""
    ctl = np.zeros((Q, counts.shape[1]), dtype=np.int64)
    np.add.at(ctl, owner, counts)
    return ctl


def query_lines(lines, names, counts, pairs, conf_sum=None, ctl=None):
    """-> the lines of query_*.txt, header first: per query the input line's chrom, start1, stop1, start2, stop2 in bp, its
    name, the bin pairs, the covered ones, the dominant state + 1 (0: nothing covered; the lowest on ties), its share, the
    entropy in bits, the mean confidence (`nan` without one), with controls the controls' total and the log2 ratio of the
    dominant state, then the K counts"""
    o = np.asarray(counts)
    mc = np.full(o.shape[0], np.nan) if conf_sum is None else mean_conf(conf_sum, o.sum(axis=-1))
    (core_head, tail_head), fields = summary_fields(o, ctl)
    head = ["#chrom", "start1", "stop1", "start2", "stop2", "name", "pairs", "covered"]
    out = ["\t".join(head + core_head + ["mean_conf"] + tail_head) + "\n"]
    for t, (chrom, s1, e1, s2, e2) in enumerate(lines):
        core, tail = fields((t,))
        f = [str(chrom), "%d" % s1, "%d" % e1, "%d" % s2, "%d" % e2, str(names[t]), "%d" % pairs[t]]
        out.append("\t".join(f + core + ["%.6f" % mc[t]] + tail) + "\n")
    return out


def query_files(path, output_path, resolution, field="state_vec", bed="", bedpe="", shift_bp=0):
    """The command line's --query: the state composition of the `field` of one estimate_ou_*.mat / segment_*.mat /
    smooth_*.mat inside the intervals of `bed` (read_intervals) or between the interval pairs of `bedpe` (read_pairs), with
    the two controls at -+ shift_bp when it is not 0.  Writes under output_path query_<stem>.npz (counts [N, K], pairs,
    covered, mean_conf when the file has conf, with a shift ctl [N, K] -- the two controls' counts summed --, ctl_covered and
    log2_ratio, queries, names, skipped_lines, K, shift in bins, len_vec and the settings; no pickles) and query_<stem>.txt
    (query_lines: one line per input line, in input order).  -> the .npz"""
    res = check_resolution(resolution)
    if bool(bed) == bool(bedpe):
        raise ValueError("query_files takes a bed file or a bedpe file, one of the two")
    shift = check_shift(res, shift_bp)
    s, L, conf = load_map(path, field)
    read = read_intervals(bed, L, res) if bed else read_pairs(bedpe, L, res)
    q = read["queries"]
    N, K = q.shape[0], (int(s.max()) + 1 if s.size else 1)
    if shift:
        controls, owner = with_controls(q, shift)
        q = np.concatenate([q, controls])
    result = state_query(s, L, q, K=K, conf=conf)
    counts, pairs = result["counts"][:N], result["pairs"][:N]
    conf_sum = None if conf is None else result["conf_sum"][:N]
    extra, ctl = {}, None
    if shift:
        ctl = control_counts(result["counts"][N:], owner, N)
        extra = dict(ctl=ctl, ctl_covered=ctl.sum(axis=1), log2_ratio=log2_ratio(counts, ctl))
    if conf is not None:
        extra["mean_conf"] = mean_conf(conf_sum, result["covered"][:N])
    os.makedirs(output_path, exist_ok=True)
    name = stem(path)
    out = os.path.join(output_path, "query_%s.npz" % name)
    np.savez(out, counts=counts, pairs=pairs, covered=result["covered"][:N], queries=read["queries"], names=np.array(read["names"], dtype=str),
             skipped_lines=np.int64(read["skipped_lines"]), K=np.int64(K), shift=np.int64(shift), len_vec=L,
             rects_region=result["rects_region"], resolution=np.int64(res), query_field=np.array(field),
             intervals=np.array(os.path.basename(bed or bedpe)), interval_kind=np.array("bed" if bed else "bedpe"),
             shift_bp=np.int64(shift_bp), **extra)
    with open(os.path.join(output_path, "query_%s.txt" % name), "wb") as fh:
        fh.write("".join(query_lines(read["lines"], read["names"], counts, pairs, conf_sum, ctl)).encode())
    return out
