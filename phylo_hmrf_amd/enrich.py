"""State enrichment between annotated genome classes: which states link which kinds of bins -- A-A
against A-B compartment bins, bin pairs inside one TAD against pairs across a TAD border -- as observed counts against an
expectation MATCHED BY EXACT GENOMIC DISTANCE.  The state of a bin pair depends steeply on its distance and two bins of one
interval are close, so a plain contingency table would call every near-diagonal state "enriched inside TADs" on every map.

Every bin carries a class (u8, 0: unannotated) and optionally a segment (int32, -1: none).  A stored node (i, j) of a region
has the pair category p = (class[i] C + class[j]) 2 + same, same = 1 when both bins lie in one segment: P = 2 C C categories.
`pair_enrichment(state_vec, len_vec, bin_class, bin_seg=None, window=(0, -1), K=None, C=None)` counts on the GPU, region by
region (phmrf_pair_enrichment, csrc/enrich.hip), obs[p][k], state_dist[d][k] and cat_dist[d][p] over the nodes inside the
distance window, sums them over the regions on one distance axis, and forms on the host, in float64,

    expected[p][k] = sum over d with N[d] > 0 of cat_dist[d][p] state_dist[d][k] / N[d],    N[d] = sum_k state_dist[d][k]

which has both margins of obs, and log2_enrichment = log2(obs / expected + 1e-16) (NaN where expected == 0).
`read_annotation(...)` reads a BED-like file into per-bin classes and segments, `fold_pairs(...)` gives the unordered view of a
table, `enrich_lines(...)` the text, `enrich_files(...)` is the command line's --enrich FILE.mat.

`enrichment_null(...)` adds the permutation null ("The enrichment's null"): the state map stays, the
annotation of every chromosome is moved by T circular shifts, and every shift is recounted on the GPU with its own
distance-matched expectation in 2^-24 fixed point (phmrf_pair_enrichment_null, csrc/enrich_null.hip); `weights`,
`expected_fixed`, `draw_shifts` and `null_statistics` are its host parts, `null_lines(...)` the text of --enrich_null.

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

from .intervals import held_chrom, interval_lines, name_group
from .maps import MAX_STATES, check_K, check_len_vec, check_resolution, check_state_vec, device, load_map, stem
from .tracks import check_windows, covered_bins, parse_windows

GRID_CAP = 1024                  # csrc/enrich.hip ENRICH_GRID_CAP: workgroups (of 256 lanes) of its kernels
TILE_H = 32                      # csrc/enrich.hip ENRICH_TILE_H: storage rows of the tile a workgroup counts at a time ...
TILE_W = 128                     # ... and ENRICH_TILE_W, its storage columns
CHUNK = 512                      # csrc/enrich.hip ENRICH_CHUNK: cells of a diagonal a wave of the class kernel takes at a time
MAX_CLASSES = 8                  # C <= 8: class 0 (none) and at most 7 names
WEIGHT_ONE = 1 << 24             # the fixed point of the null's weights and expectations (maps.CONF_ONE's scale)
NULL_MAX_SHIFTS = 4096           # csrc/enrich_null.hip NULL_MAX_SHIFTS: shifts of one phmrf_pair_enrichment_null call
NULL_TABLE_LIMIT = 1 << 26       # T 2 C C K stays below it (include/phmrf.h, phmrf_pair_enrichment_null)
NULL_LDS_BYTES = 65536           # csrc/enrich_null.hip NULL_LDS_BYTES: LDS of the null's counting kernel ...
NULL_MAX_GROUP = 16              # ... and NULL_MAX_GROUP, the shifts a workgroup counts a tile against at most (null_group)
NULL_GRID_CAP = 1024             # csrc/enrich_null.hip NULL_GRID_CAP: workgroups of the counting kernel
NULL_CLASS_CAP = 4096            # csrc/enrich_null.hip NULL_CLASS_CAP: workgroups of the expectation kernel
NULL_CHUNK = 512                 # csrc/enrich_null.hip NULL_CHUNK: cells of a diagonal a wave of the expectation kernel takes
HEADER = "#class_a\tclass_b\tsame\tstate\tobserved\texpected\tlog2_enrichment\tshare_of_category\tshare_of_state"
NULL_HEADER = ("#class_a\tclass_b\tsame\tstate\tobserved\texpected\tnull_mean_excess\tnull_sd_excess\tz\tp_low\tp_high\tp")
STATISTICS = ("null_mean", "null_sd", "z", "p_high", "p_low", "p")


def null_group(K, C):
    """csrc/enrich_null.hip null_group_shifts: the shifts TS a workgroup of the null's counting kernel counts a tile against,
    as many u32 [2 C C][K] count tables plus 8 bytes for each of the tile's TILE_H + TILE_W bins as fit NULL_LDS_BYTES, at
    least 1 and at most NULL_MAX_GROUP"""
    per = 4 * 2 * int(C) * int(C) * int(K) + 8 * (TILE_H + TILE_W)
    return max(1, min(NULL_MAX_GROUP, NULL_LDS_BYTES // per))


def distance_range(H, W, diagonal, dist0, d_min, d_max):
    """-> (d_lo, D): the distances |dist0 + j - i| of an H x W region (a diagonal block: its stored nodes, j >= i) that lie
    inside the window d_min <= d and (d_max == -1 or d <= d_max) are d_lo .. d_lo + D - 1; None when no cell is inside"""
    H, W, dist0, d_min, d_max = int(H), int(W), int(dist0), int(d_min), int(d_max)
    x_lo, x_hi = (0, H - 1) if diagonal else (dist0 - (H - 1), dist0 + W - 1)
    near = 0 if x_lo <= 0 <= x_hi else min(abs(x_lo), abs(x_hi))
    far = max(abs(x_lo), abs(x_hi))
    lo, hi = max(near, d_min), far if d_max == -1 else min(far, d_max)
    return (lo, hi - lo + 1) if lo <= hi else None


def expected(state_dist, cat_dist):
    """state_dist [D, K], cat_dist [D, P] on one distance axis -> float64 [P, K]: the counts of every category and state if,
    at every distance, the categories' nodes drew their states from that distance's composition.  Host only."""
    S, Cat = np.asarray(state_dist, dtype=np.float64), np.asarray(cat_dist, dtype=np.float64)
    if S.ndim != 2 or Cat.ndim != 2 or S.shape[0] != Cat.shape[0]:
        raise ValueError("expected takes state_dist [D, K] and cat_dist [D, P] on one distance axis")
    N = S.sum(axis=1)
    full = N > 0
    return Cat[full].T @ (S[full] / N[full, None])


def log2_enrichment(obs, exp):
    """-> log2(obs / exp + 1e-16), NaN where exp == 0.  Host only."""
    obs, exp = np.asarray(obs, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    out = np.full(obs.shape, np.nan)
    np.log2(np.divide(obs, exp, out=np.zeros(obs.shape), where=exp > 0) + 1e-16, out=out, where=exp > 0)
    return out


def fold_pairs(table, C):
    """table [2 C C, ...] over the ORDERED pair categories -> [C, C, 2, ...] over the unordered ones: [a][b] with a < b is
    (a, b) plus (b, a), [a][a] is (a, a), [a][b] with a > b is zero.  Host only."""
    t = np.asarray(table)
    C = int(C)
    if t.ndim < 1 or t.shape[0] != 2 * C * C:
        raise ValueError("fold_pairs takes a table whose first axis is the 2 C C = %d pair categories" % (2 * C * C))
    t = t.reshape((C, C, 2) + t.shape[1:])
    out = np.zeros_like(t)
    for a in range(C):
        out[a, a] = t[a, a]
        for b in range(a + 1, C):
            out[a, b] = t[a, b] + t[b, a]
    return out


def read_annotation(path, len_vec, resolution, segments=False):
    """A BED-like text file `chrom start stop name` (tabs or spaces; lines that start with # and blank lines are skipped) ->
    dict:
      bin_class {chrom: u8 [B]}       per bin of every chromosome of len_vec (B: the bins its regions reach) its class
      bin_seg {chrom: int32 [B]}      with segments: the index, among the kept lines, of the line that gave the class; -1 for
                                      an unannotated bin.  None without segments
      names                           ["none", the distinct names of the file in order of first appearance]: class c is names[c]
      skipped_lines                   the lines of other chromosomes
    chrom is chr<N> or <N>, N the integer in len_vec's column 9.  A bin g takes the FIRST line in file order whose
    [start, stop) holds its midpoint g res + res // 2.  The names are numbered over the whole file, whatever chromosomes
    len_vec holds.  ValueError for a malformed line, start >= stop, a negative coordinate and more than 7 names.  Host only."""
    res = check_resolution(resolution)
    L = np.asarray(len_vec)
    bin_class = {int(c): np.zeros(covered_bins(L, c).shape[0], dtype=np.uint8) for c in np.unique(L[:, 9])}
    bin_seg = {c: np.full(v.shape[0], -1, dtype=np.int32) for c, v in bin_class.items()} if segments else None
    taken = {c: np.zeros(v.shape[0], dtype=bool) for c, v in bin_class.items()}
    names, skipped, kept = [], 0, 0                           # (the file's names: class 0, `none`, is not among them)
    why = ": at most %d classes beside `none` are supported" % (MAX_CLASSES - 1)
    for number, _, chroms, ((start, stop),), rest in interval_lines(path, 1, "chrom start stop name", False, fields=4):
        cls = 1 + name_group(path, number, names, rest[0], MAX_CLASSES - 1, why)
        c = held_chrom(chroms, bin_class)
        if c is None:
            skipped += 1
            continue
        B, half = bin_class[c].shape[0], res // 2
        g0 = min(B, max(0, -(-(start - half) // res)))          # the first g with g res + half >= start
        g1 = min(B, max(0, -(-(stop - half) // res)))           # the first g with g res + half >= stop
        if g1 > g0:
            free = ~taken[c][g0:g1]
            bin_class[c][g0:g1][free] = cls
            if segments:
                bin_seg[c][g0:g1][free] = kept
            taken[c][g0:g1] = True
        kept += 1
    return dict(bin_class=bin_class, bin_seg=bin_seg, names=["none"] + names, skipped_lines=skipped)


def _slice(table, chrom, start, count, fill, dtype):
    """bins [start, start + count) of the chromosome's array; a missing chromosome and bins beyond the array's end: fill"""
    out = np.full(count, fill, dtype=dtype)
    a = None if table is None else table.get(int(chrom))
    if a is not None:
        part = np.asarray(a).reshape(-1)[start:start + count]
        out[:part.shape[0]] = part
    return out


def _int_table(d, what, lo, hi):
    if d is None:
        return None
    out = {}
    for c, v in dict(d).items():
        v = np.asarray(v).reshape(-1)
        if v.dtype.kind not in "iu" or (v.size and (int(v.min()) < lo or int(v.max()) > hi)):
            raise ValueError("%s of chromosome %s must hold integers in %d .. %d" % (what, c, lo, hi))
        out[int(c)] = v
    return out


def pair_enrichment(state_vec, len_vec, bin_class, bin_seg=None, window=(0, -1), K=None, C=None):
    """bin_class {chrom: [B] classes 0 .. C - 1}, bin_seg {chrom: [B] segments, -1: none} or None -> dict:
      obs int64 [P, K]                  the nodes inside the window of pair category p in state k, all regions; P = 2 C C
      obs_region int64 [R, P, K]        the same per region
      state_dist int64 [Dg, K]          the nodes at the distance d0 + t in state k, all regions
      cat_dist int64 [Dg, P]            the nodes at the distance d0 + t of category p, all regions
      d0 int64                          the first distance of the axis (Dg = 0: no node is inside the window)
      expected float64 [P, K]           expected(state_dist, cat_dist)
      log2_enrichment float64 [P, K]    log2(obs / expected + 1e-16), NaN where expected == 0
      window int64 [2], K, C
    A chromosome that bin_class (bin_seg) does not hold, and bins beyond an array's end, are class 0 (segment -1).  A node
    (i, j) of a region has the distance |start_bin2 - start_bin1 + j - i|; window = (d_min, d_max) in bins, d_max -1: no upper
    limit.  Stored nodes count once.  K: the largest state + 1 by default, C: the largest class + 1; a state >= K inside the
    window is an error, outside it is not looked at."""
    from . import _lib
    import torch
    s = check_state_vec(state_vec)
    L = check_len_vec(len_vec, s.shape[0])
    d_min, d_max = (int(x) for x in check_windows([tuple(window)])[0])
    K = check_K(s, K)
    classes = _int_table(bin_class, "bin_class", 0, 255)
    segs = _int_table(bin_seg, "bin_seg", -1, 2 ** 31 - 1)
    C = max([1] + [int(v.max()) + 1 for v in classes.values() if v.size]) if C is None else int(C)
    if C < 1 or C > MAX_CLASSES:
        raise ValueError("C must be in 1 .. %d (class 0 and at most %d names)" % (MAX_CLASSES, MAX_CLASSES - 1))
    lib, dev, stream = device()
    P = 2 * C * C
    ranges = [distance_range(r[3], r[4], int(r[8]), int(r[6]) - int(r[5]), d_min, d_max) for r in L]
    held = [g for g in ranges if g is not None]
    d0 = min([g[0] for g in held]) if held else d_min
    Dg = max([g[0] + g[1] for g in held]) - d0 if held else 0
    obs_region = np.zeros((L.shape[0], P, K), dtype=np.int64)
    state_dist = np.zeros((Dg, K), dtype=np.int64)
    cat_dist = np.zeros((Dg, P), dtype=np.int64)
    s_t = torch.from_numpy(s.astype(np.uint8)).to(dev)
    for r, row in enumerate(L):
        if ranges[r] is None:
            continue
        lo, hi, H, W, s1, s2, diag, chrom = (int(row[x]) for x in (1, 2, 3, 4, 5, 6, 8, 9))
        d_lo, D = ranges[r]
        cls = np.concatenate([_slice(classes, chrom, s1, H, 0, np.uint8), _slice(classes, chrom, s2, W, 0, np.uint8)])
        cls_t = torch.from_numpy(cls).to(dev)
        seg_t = None
        if segs is not None:
            seg_t = torch.from_numpy(np.concatenate([_slice(segs, chrom, s1, H, -1, np.int32),
                                                     _slice(segs, chrom, s2, W, -1, np.int32)])).to(dev)
        sd, cd = np.zeros((D, K), dtype=np.int64), np.zeros((D, P), dtype=np.int64)
        _lib.check(lib.phmrf_pair_enrichment(
            ctypes.c_void_p(s_t[lo:hi].data_ptr()), H, W, diag, s2 - s1, K, C, ctypes.c_void_p(cls_t.data_ptr()),
            ctypes.c_void_p(cls_t[H:].data_ptr()), None if seg_t is None else ctypes.c_void_p(seg_t.data_ptr()),
            None if seg_t is None else ctypes.c_void_p(seg_t[H:].data_ptr()), d_min, d_max, d_lo, D,
            _lib.ptr_i64(obs_region[r]), _lib.ptr_i64(sd), _lib.ptr_i64(cd), stream))
        state_dist[d_lo - d0:d_lo - d0 + D] += sd
        cat_dist[d_lo - d0:d_lo - d0 + D] += cd
    obs = obs_region.sum(axis=0)
    exp = expected(state_dist, cat_dist)
    return dict(obs=obs, obs_region=obs_region, state_dist=state_dist, cat_dist=cat_dist, d0=np.int64(d0), expected=exp,
                log2_enrichment=log2_enrichment(obs, exp), window=np.array([d_min, d_max], dtype=np.int64), K=np.int64(K),
                C=np.int64(C))


def weights(state_dist):
    """state_dist int [Dg, K] -> uint32 [Dg, K]: w[d][k] = (S[d][k] WEIGHT_ONE) // N[d], N[d] = sum_k S[d][k], by exact integer
    floor division; a row with N[d] = 0 is zero.  Every entry is <= WEIGHT_ONE.  Host only."""
    S = np.asarray(state_dist)
    if S.ndim != 2 or S.dtype.kind not in "iu" or (S.size and int(S.min()) < 0):
        raise ValueError("weights takes a table of non-negative integer counts [Dg, K]")
    S = S.astype(np.int64)
    N = S.sum(axis=1)
    if N.size and int(N.max()) >= (1 << 63) // WEIGHT_ONE:
        raise ValueError("a distance holds 2^39 nodes or more: its counts times 2^24 do not fit 63 bits")
    w = np.zeros(S.shape, dtype=np.uint32)
    full = N > 0
    w[full] = (S[full] * WEIGHT_ONE) // N[full, None]
    return w


def expected_fixed(cat_dist, w):
    """cat_dist int [Dg, P], w = weights(state_dist) [Dg, K] -> int64 [P, K]: expq[p][k] = sum_d cat_dist[d][p] w[d][k], an
    exact integer matrix product; the expectation in units of 1 / WEIGHT_ONE, with
    0 <= expected[p][k] WEIGHT_ONE - expq[p][k] <= sum_d cat_dist[d][p] up to float64 rounding.  Host only."""
    Cat, w = np.asarray(cat_dist), np.asarray(w)
    if Cat.ndim != 2 or w.ndim != 2 or Cat.shape[0] != w.shape[0] or Cat.dtype.kind not in "iu" or w.dtype.kind not in "iu":
        raise ValueError("expected_fixed takes integer tables cat_dist [Dg, P] and w [Dg, K] on one distance axis")
    return Cat.astype(np.int64).T @ w.astype(np.int64)


def draw_shifts(len_vec, n, min_shift=0, seed=0):
    """-> {chrom: int64 [n]}: n circular shifts per chromosome of len_vec from np.random.default_rng(seed), the chromosomes in
    ascending order; chromosome c with B_c bins (tracks.covered_bins) draws uniformly from [m_c, B_c - m_c] with
    m_c = min(min_shift, B_c // 2), reduced mod B_c.  Host only."""
    n, min_shift = int(n), int(min_shift)
    if n < 1 or min_shift < 0:
        raise ValueError("draw_shifts takes n >= 1 and min_shift >= 0")
    L = np.asarray(len_vec)
    rng = np.random.default_rng(seed)
    out = {}
    for c in sorted(int(x) for x in np.unique(L[:, 9])):
        B = int(covered_bins(L, c).shape[0])
        m = min(min_shift, B // 2)
        out[c] = rng.integers(m, B - m + 1, n).astype(np.int64) % max(B, 1)
    return out


def null_statistics(obs, expq, null_obs, null_expq, C):
    """obs, expq int [P, K] of the unshifted annotation and null_obs, null_expq int [T, P, K] of the T draws -> dict of
    float64 [C, C, 2, K] over the unordered categories (fold_pairs).  With the excess x = obs WEIGHT_ONE - expq, an exact
    int64, x_0 the unshifted one and x_t the draws':
      null_mean, null_sd   of x_t / WEIGHT_ONE over t (the sd with T - 1 in the denominator: NaN for T = 1)
      z                    (x_0 / WEIGHT_ONE - null_mean) / null_sd, NaN where null_sd == 0
      p_high, p_low        (1 + #{t: x_t >= x_0}) / (T + 1), (1 + #{t: x_t <= x_0}) / (T + 1): compared on the integers
      p                    min(1, 2 min(p_high, p_low))
    Host only."""
    C = int(C)
    o, e = np.asarray(obs), np.asarray(expq)
    no, ne = np.asarray(null_obs), np.asarray(null_expq)
    if any(a.dtype.kind not in "iu" for a in (o, e, no, ne)):
        raise ValueError("null_statistics takes integer tables")
    if o.shape != e.shape or no.shape != ne.shape or no.ndim != o.ndim + 1 or no.shape[1:] != o.shape or no.shape[0] < 1:
        raise ValueError("null_statistics takes obs, expq [P, K] and null_obs, null_expq [T, P, K] with T >= 1")
    x0 = fold_pairs(o.astype(np.int64) * WEIGHT_ONE - e.astype(np.int64), C)
    xt = np.moveaxis(fold_pairs(np.moveaxis(no.astype(np.int64) * WEIGHT_ONE - ne.astype(np.int64), 0, -1), C), -1, 0)
    T = xt.shape[0]
    f = xt.astype(np.float64) / WEIGHT_ONE
    mean = f.mean(axis=0)
    sd = f.std(axis=0, ddof=1) if T > 1 else np.full(mean.shape, np.nan)
    z = np.full(mean.shape, np.nan)
    np.divide(x0.astype(np.float64) / WEIGHT_ONE - mean, sd, out=z, where=sd > 0)
    p_high = (1 + (xt >= x0[None]).sum(axis=0)) / (T + 1.0)
    p_low = (1 + (xt <= x0[None]).sum(axis=0)) / (T + 1.0)
    return dict(null_mean=mean, null_sd=sd, z=z, p_high=p_high, p_low=p_low, p=np.minimum(1.0, 2.0 * np.minimum(p_high, p_low)))


class NullSizeError(ValueError):
    """the null's tables would hold NULL_TABLE_LIMIT entries or more"""


def check_null_size(n, K, C):
    """ValueError unless 1 <= n, NullSizeError unless n 2 C C K < NULL_TABLE_LIMIT: the null's two tables int64 [n, 2 C C, K]"""
    n, K, C = int(n), int(K), int(C)
    if n < 1:
        raise ValueError("the null takes at least one shift")
    if n * 2 * C * C * K >= NULL_TABLE_LIMIT:
        raise NullSizeError("%d shifts with K = %d states and C = %d classes: n 2 C C K = %d must stay below 2^26"
                         % (n, K, C, n * 2 * C * C * K))


def enrichment_null(state_vec, len_vec, bin_class, bin_seg=None, window=(0, -1), K=None, C=None, shifts=None, n=1000,
                    min_shift=0, seed=0, _max_call=NULL_MAX_SHIFTS):
    """pair_enrichment(...) and its permutation null -> pair_enrichment's dict plus
      weights uint32 [Dg, K]            weights(state_dist): the state map does not move, so they serve every draw
      expq int64 [P, K]                 expected_fixed(cat_dist, weights): the unshifted expectation in units of 1 / WEIGHT_ONE
      null_obs, null_expq int64 [T, P, K]   the same two tables under draw t, summed over the regions
      shifts {chrom: int64 [T]}         draw t moves chromosome c by shifts[c][t]: class_s[g] = class[(g + s) mod B_c]
      null_mean, null_sd, z, p_high, p_low, p    null_statistics(...), float64 [C, C, 2, K]
    Chromosome c has B_c = len(tracks.covered_bins(len_vec, c)) bins; its class and segment arrays are padded with class 0 /
    segment -1, or cut, to B_c and uploaded once.  shifts: given explicitly ({chrom: [T] in 0 .. B_c - 1} for every
    chromosome of len_vec, one length) it overrides n, min_shift and seed, which go to draw_shifts otherwise.  Every region
    takes one phmrf_pair_enrichment_null call per _max_call shifts (a test's argument: at most NULL_MAX_SHIFTS) with its slice
    of the weights.  RuntimeError without a GPU: there is no host fallback."""
    from . import _lib
    import torch
    res = pair_enrichment(state_vec, len_vec, bin_class, bin_seg, window=window, K=K, C=C)
    K, C = int(res["K"]), int(res["C"])
    d_min, d_max = (int(x) for x in res["window"])
    s = check_state_vec(state_vec)
    L = check_len_vec(len_vec, s.shape[0])
    if s.shape[0] >= (1 << 63) // WEIGHT_ONE:
        raise ValueError("a map of 2^39 nodes or more: its counts times 2^24 do not fit 63 bits")
    chroms = sorted(int(c) for c in np.unique(L[:, 9]))
    bins = {c: int(covered_bins(L, c).shape[0]) for c in chroms}
    if shifts is None:
        shifts = draw_shifts(L, n, min_shift=min_shift, seed=seed)
    else:
        shifts = {int(c): np.asarray(v).reshape(-1) for c, v in dict(shifts).items()}
        if sorted(shifts) != chroms:
            raise ValueError("shifts must hold one array for every chromosome of len_vec: %s" % chroms)
        for c, v in shifts.items():
            if v.dtype.kind not in "iu" or (v.size and (int(v.min()) < 0 or int(v.max()) >= bins[c])):
                raise ValueError("shifts of chromosome %d must be integers in 0 .. %d" % (c, bins[c] - 1))
        shifts = {c: v.astype(np.int64) for c, v in shifts.items()}
    T = int(shifts[chroms[0]].shape[0]) if chroms else 0
    if T < 1 or any(v.shape[0] != T for v in shifts.values()):
        raise ValueError("shifts must hold arrays of one length >= 1")
    check_null_size(T, K, C)
    _max_call = int(_max_call)
    if not 1 <= _max_call <= NULL_MAX_SHIFTS:
        raise ValueError("_max_call must be in 1 .. %d" % NULL_MAX_SHIFTS)
    lib, dev, stream = device()
    classes = _int_table(bin_class, "bin_class", 0, 255)
    segs = _int_table(bin_seg, "bin_seg", -1, 2 ** 31 - 1)
    P = 2 * C * C
    w = weights(res["state_dist"])
    d0 = int(res["d0"])
    cls_t = {c: torch.from_numpy(_slice(classes, c, 0, bins[c], 0, np.uint8)).to(dev) for c in chroms}
    seg_t = None if segs is None else {c: torch.from_numpy(_slice(segs, c, 0, bins[c], -1, np.int32)).to(dev) for c in chroms}
    shifts32 = {c: np.ascontiguousarray(v, dtype=np.int32) for c, v in shifts.items()}
    s_t = torch.from_numpy(s.astype(np.uint8)).to(dev)
    null_obs, null_expq = np.zeros((T, P, K), dtype=np.int64), np.zeros((T, P, K), dtype=np.int64)
    for row in L:
        lo, hi, H, W, s1, s2, diag, chrom = (int(row[x]) for x in (1, 2, 3, 4, 5, 6, 8, 9))
        rng = distance_range(H, W, diag, s2 - s1, d_min, d_max)
        if rng is None:
            continue
        d_lo, D = rng
        w_r = np.ascontiguousarray(w[d_lo - d0:d_lo - d0 + D])
        for a in range(0, T, _max_call):
            tc = min(_max_call, T - a)
            ob, eq = np.zeros((tc, P, K), dtype=np.int64), np.zeros((tc, P, K), dtype=np.int64)
            _lib.check(lib.phmrf_pair_enrichment_null(
                ctypes.c_void_p(s_t[lo:hi].data_ptr()), H, W, diag, s1, s2, K, C, ctypes.c_void_p(cls_t[chrom].data_ptr()),
                None if seg_t is None else ctypes.c_void_p(seg_t[chrom].data_ptr()), bins[chrom],
                _lib.ptr_i32(shifts32[chrom][a:a + tc]), tc, d_min, d_max, d_lo, D,
                w_r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _lib.ptr_i64(ob), _lib.ptr_i64(eq), stream))
            null_obs[a:a + tc] += ob
            null_expq[a:a + tc] += eq
    expq = expected_fixed(res["cat_dist"], w)
    out = dict(res, weights=w, expq=expq, null_obs=null_obs, null_expq=null_expq, shifts=shifts)
    out.update(null_statistics(res["obs"], expq, null_obs, null_expq, C))
    return out


def null_lines(result, names):
    """-> the lines of enrich_*_null.txt from enrichment_null's dict, NULL_HEADER first: enrich_lines' rows (one per unordered
    class pair, `same` flag and state of the categories that hold a node) with observed, expected (expq / WEIGHT_ONE), the
    null's mean and sd of the excess observed - expected, z, p_low, p_high and p"""
    C, K = int(result["C"]), int(result["K"])
    obs, exp = fold_pairs(result["obs"], C), fold_pairs(result["expq"], C).astype(np.float64) / WEIGHT_ONE
    name = lambda c: names[c] if c < len(names) else "class%d" % c
    lines = [NULL_HEADER + "\n"]
    for a in range(C):
        for b in range(a, C):
            for same in (0, 1):
                if not int(obs[a, b, same].sum()):
                    continue
                for k in range(K):
                    at = (a, b, same, k)
                    lines.append("%s\t%s\t%d\t%d\t%d\t%.3f\t%.3f\t%.3f\t%.4f\t%.6f\t%.6f\t%.6f\n"
                                 % (name(a), name(b), same, k + 1, int(obs[at]), exp[at], result["null_mean"][at],
                                    result["null_sd"][at], result["z"][at], result["p_low"][at], result["p_high"][at],
                                    result["p"][at]))
    return lines


def enrich_lines(result, names):
    """-> the lines of enrich_*.txt from pair_enrichment's dict, header first: one line per unordered class pair a <= b
    (fold_pairs), `same` flag and state, for the categories that hold a node: class_a, class_b, same, state + 1, observed,
    expected, log2 enrichment (of the folded counts), the state's share of the category, the category's share of the state
    (of the state's nodes inside the window)."""
    C, K = int(result["C"]), int(result["K"])
    obs, exp = fold_pairs(result["obs"], C), fold_pairs(result["expected"], C)
    l2 = log2_enrichment(obs, exp)
    per_state = np.asarray(result["obs"]).sum(axis=0)
    name = lambda c: names[c] if c < len(names) else "class%d" % c
    lines = [HEADER + "\n"]
    for a in range(C):
        for b in range(a, C):
            for same in (0, 1):
                total = int(obs[a, b, same].sum())
                if not total:
                    continue
                for k in range(K):
                    o = int(obs[a, b, same, k])
                    lines.append("%s\t%s\t%d\t%d\t%d\t%.3f\t%.4f\t%.6f\t%.6f\n"
                                 % (name(a), name(b), same, k + 1, o, exp[a, b, same, k], l2[a, b, same, k], o / total,
                                    o / per_state[k] if per_state[k] else np.nan))
    return lines


def enrich_files(path, bed, output_path, resolution, field="state_vec", window_bp="0-", segments=False, null=0,
                 null_min_bp=1000000, null_seed=0):
    """The command line's --enrich: count the `field` of one estimate_ou_*.mat / segment_*.mat / smooth_*.mat against the
    annotation file `bed`.  Writes under output_path enrich_<stem>.npz (pair_enrichment's arrays, names, skipped_lines,
    class_<chrom> and seg_<chrom>, len_vec, resolution, enrich_field, window_bp, segments; no pickles) and enrich_<stem>.txt
    (enrich_lines).  null > 0 (--enrich_null): enrichment_null with that many shifts of at least max(1, null_min_bp //
    resolution) bins drawn with null_seed; the .npz gains its arrays (shifts_<chrom> per chromosome), null_min_bp and
    null_seed, and enrich_<stem>_null.txt (null_lines) is written beside the unchanged enrich_<stem>.txt.  -> the .npz"""
    res = int(resolution)
    if res < 1:
        raise ValueError("resolution must be >= 1")
    wins = parse_windows(window_bp, res)
    if len(wins) != 1:
        raise ValueError("expected one window lo-hi or lo-, got %r" % (window_bp,))
    s, L, _ = load_map(path, field)
    ann = read_annotation(bed, L, res, segments=bool(segments))
    null = int(null)
    if null < 0:
        raise ValueError("null must be >= 0")
    extra = {}
    if null:
        states = check_state_vec(s)
        check_null_size(null, int(states.max()) + 1 if states.size else 1, len(ann["names"]))
        result = enrichment_null(s, L, ann["bin_class"], ann["bin_seg"], window=wins[0], C=len(ann["names"]), n=null,
                                 min_shift=max(1, int(null_min_bp) // res), seed=int(null_seed))
        extra.update({"shifts_%d" % c: v for c, v in result.pop("shifts").items()})
        extra.update(null_min_bp=np.int64(null_min_bp), null_seed=np.int64(null_seed))
    else:
        result = pair_enrichment(s, L, ann["bin_class"], ann["bin_seg"], window=wins[0], C=len(ann["names"]))
    os.makedirs(output_path, exist_ok=True)
    name = stem(path)
    out = os.path.join(output_path, "enrich_%s.npz" % name)
    extra.update({"class_%d" % c: v for c, v in ann["bin_class"].items()})
    if ann["bin_seg"] is not None:
        extra.update({"seg_%d" % c: v for c, v in ann["bin_seg"].items()})
    np.savez(out, len_vec=L, resolution=np.int64(res), enrich_field=np.array(field), window_bp=np.array(str(window_bp)),
             segments=np.int64(bool(segments)), names=np.array(ann["names"]), skipped_lines=np.int64(ann["skipped_lines"]),
             **extra, **result)
    with open(os.path.join(output_path, "enrich_%s.txt" % name), "wb") as fh:
        fh.write("".join(enrich_lines(result, ann["names"])).encode())
    if null:
        with open(os.path.join(output_path, "enrich_%s_null.txt" % name), "wb") as fh:
            fh.write("".join(null_lines(result, ann["names"])).encode())
    return out
