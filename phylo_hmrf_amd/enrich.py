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

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

from .maps import MAX_STATES, check_len_vec, check_state_vec, chrom_of, device, load_map, stem
from .tracks import check_windows, covered_bins, parse_windows

GRID_CAP = 1024                  # csrc/enrich.hip ENRICH_GRID_CAP: workgroups (of 256 lanes) of its kernels
TILE_H = 32                      # csrc/enrich.hip ENRICH_TILE_H: storage rows of the tile a workgroup counts at a time ...
TILE_W = 128                     # ... and ENRICH_TILE_W, its storage columns
CHUNK = 512                      # csrc/enrich.hip ENRICH_CHUNK: cells of a diagonal a wave of the class kernel takes at a time
MAX_CLASSES = 8                  # C <= 8: class 0 (none) and at most 7 names
HEADER = "#class_a\tclass_b\tsame\tstate\tobserved\texpected\tlog2_enrichment\tshare_of_category\tshare_of_state"


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


_chrom_of = chrom_of


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
    res = int(resolution)
    if res < 1:
        raise ValueError("resolution must be >= 1")
    L = np.asarray(len_vec)
    bin_class = {int(c): np.zeros(covered_bins(L, c).shape[0], dtype=np.uint8) for c in np.unique(L[:, 9])}
    bin_seg = {c: np.full(v.shape[0], -1, dtype=np.int32) for c, v in bin_class.items()} if segments else None
    taken = {c: np.zeros(v.shape[0], dtype=bool) for c, v in bin_class.items()}
    names, skipped, kept = ["none"], 0, 0
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            f = line.split()
            if not f or f[0].startswith("#"):
                continue
            if len(f) < 4 or not f[1].lstrip("-").isdigit() or not f[2].lstrip("-").isdigit():
                raise ValueError("%s line %d: expected `chrom start stop name`, got %r" % (path, number, line.rstrip("\n")))
            start, stop = int(f[1]), int(f[2])
            if start < 0 or stop < 0:
                raise ValueError("%s line %d: negative coordinate" % (path, number))
            if start >= stop:
                raise ValueError("%s line %d: start %d >= stop %d" % (path, number, start, stop))
            if f[3] not in names[1:]:
                if len(names) == MAX_CLASSES:
                    raise ValueError("%s line %d: more than %d names (%s, then %r): at most %d classes beside `none` are "
                                     "supported" % (path, number, MAX_CLASSES - 1, ", ".join(names[1:]), f[3], MAX_CLASSES - 1))
                names.append(f[3])
            c = _chrom_of(f[0])
            if c not in bin_class:
                skipped += 1
                continue
            B, half = bin_class[c].shape[0], res // 2
            g0 = min(B, max(0, -(-(start - half) // res)))          # the first g with g res + half >= start
            g1 = min(B, max(0, -(-(stop - half) // res)))           # the first g with g res + half >= stop
            if g1 > g0:
                free = ~taken[c][g0:g1]
                bin_class[c][g0:g1][free] = names.index(f[3], 1)
                if segments:
                    bin_seg[c][g0:g1][free] = kept
                taken[c][g0:g1] = True
            kept += 1
    return dict(bin_class=bin_class, bin_seg=bin_seg, names=names, skipped_lines=skipped)


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
    K = (int(s.max()) + 1 if s.size else 1) if K is None else int(K)
    if K < 1 or K > MAX_STATES:
        raise ValueError("K must be in 1 .. %d" % MAX_STATES)
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


def enrich_files(path, bed, output_path, resolution, field="state_vec", window_bp="0-", segments=False):
    """The command line's --enrich: count the `field` of one estimate_ou_*.mat / segment_*.mat / smooth_*.mat against the
    annotation file `bed`.  Writes under output_path enrich_<stem>.npz (pair_enrichment's arrays, names, skipped_lines,
    class_<chrom> and seg_<chrom>, len_vec, resolution, enrich_field, window_bp, segments; no pickles) and enrich_<stem>.txt
    (enrich_lines).  -> the .npz"""
    res = int(resolution)
    if res < 1:
        raise ValueError("resolution must be >= 1")
    wins = parse_windows(window_bp, res)
    if len(wins) != 1:
        raise ValueError("expected one window lo-hi or lo-, got %r" % (window_bp,))
    s, L, _ = load_map(path, field)
    ann = read_annotation(bed, L, res, segments=bool(segments))
    result = pair_enrichment(s, L, ann["bin_class"], ann["bin_seg"], window=wins[0], C=len(ann["names"]))
    os.makedirs(output_path, exist_ok=True)
    name = stem(path)
    out = os.path.join(output_path, "enrich_%s.npz" % name)
    extra = {"class_%d" % c: v for c, v in ann["bin_class"].items()}
    if ann["bin_seg"] is not None:
        extra.update({"seg_%d" % c: v for c, v in ann["bin_seg"].items()})
    np.savez(out, len_vec=L, resolution=np.int64(res), enrich_field=np.array(field), window_bp=np.array(str(window_bp)),
             segments=np.int64(bool(segments)), names=np.array(ann["names"]), skipped_lines=np.int64(ann["skipped_lines"]),
             **extra, **result)
    with open(os.path.join(output_path, "enrich_%s.txt" % name), "wb") as fh:
        fh.write("".join(enrich_lines(result, ann["names"])).encode())
    return out
