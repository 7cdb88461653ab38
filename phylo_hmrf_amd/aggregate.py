"""Rescaled pile-ups of a state map over features of unequal size: what does the map look like ACROSS the
body of my features -- from a TAD's left border through its interior to its right border, across a compartment domain, over
the rectangle between two domains --, averaged over features whose lengths differ by orders of magnitude.  Every feature is
stretched or shrunk onto one grid and the grids are stacked (for contact maps: aggregate TAD analysis).

A feature is (chrom, A = [a0, a1), B = [b0, b1), group, flip) in chromosome bins.  The grid has a body of T cells per axis and
a flank of F cells on either side, P = T + 2 F; the flank scales with the feature.  For an interval [x0, x1) of n >= 1 bins
    edge(c) = x0 + floor((c - F) n / T),  c = 0 .. P      (a true floor: the left flank's numerators are negative)
    cell c  = the bins [edge(c), max(edge(c) + 1, edge(c + 1)))
(`axis_cells`, the one place the rule is written in Python): the body cells tile [x0, x1) exactly when n >= T; when n < T a
cell takes the single bin that holds its left edge and neighbouring cells may repeat a bin (nearest-neighbour upsampling).
Pile cell (u, v) of a feature covers I x J, I = cell u' of A's axis and J = cell v' of B's, (u', v') = (u, v), or
(P - 1 - u, P - 1 - v) when the feature is flipped.  A stored node of any region of the chromosome stands for the bin pair
(p, q) = (start_bin1 + i, start_bin2 + j) and adds [(p, q) in I x J] + [p != q and (q, p) in I x J] to hist[f][u][v][state]:
the symmetric chromosome matrix read through all its regions at once.  Bins that no region covers are simply not counted.

`state_aggregate(state_vec, len_vec, features, body, flank, K=None, G=None)` computes on the GPU, one call per chromosome
(phmrf_state_aggregate, csrc/aggregate.hip),
    cells[g][u][v][k] = sum over the features f of group g of hist[f][u][v][k]    (bin pairs: large features weigh more)
    votes[g][u][v][k] = the features of group g whose pile cell (u, v) is not empty and has k as its most frequent state,
                        the lowest k on ties                                      (one vote a feature: all weigh the same)
`read_features(...)` reads a BED file into features with A = B, `read_feature_pairs(...)` a BEDPE file, `with_controls(...)`
adds the features shifted ALONG the diagonal, `aggregate_lines(...)` writes the text table, `aggregate_files(...)` is the
command line's --aggregate FILE.mat.

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

from .intervals import (MAX_GROUPS, MAX_NAMES, check_G, check_shift, held_chrom, held_chroms, interval_lines, log2_ratio, name_group,
                        overlap_bins, pile_summary, shift_along_diagonal, summary_fields, write_group_images)
from .maps import check_K, check_len_vec, check_resolution, check_state_vec, device, load_map, stem
from .pileup import pile_image
from .render import default_palette, load_palette

LANES = 128                      # csrc/aggregate.hip AGG_LANES: pile cells of a tile = lanes of a workgroup of the lane kernel
CHUNK = 256                      # csrc/aggregate.hip AGG_CHUNK: features of one group a workgroup piles at a time
GRID_CAP = 4096                  # csrc/aggregate.hip AGG_GRID_CAP: workgroups of the lane kernel
SMALL_AREA = 256                 # csrc/aggregate.hip AGG_SMALL_AREA: a feature with ceil(nA / T) ceil(nB / T) bin pairs a cell
#                                  above this is walked a wave per pile cell, not a lane per pile cell
WAVES = 4                        # csrc/aggregate.hip AGG_WAVES: waves of a workgroup of the wave kernel
WAVE_GRID_CAP = 2048             # csrc/aggregate.hip AGG_WAVE_GRID_CAP: workgroups of the wave kernel
MAX_BODY = 64                    # csrc/aggregate.hip AGG_MAX_BODY: T <= 64
MAX_FLANK = 32                   # csrc/aggregate.hip AGG_MAX_FLANK: F <= 32
MAX_REGIONS = 64                 # csrc/aggregate.hip AGG_MAX_REGIONS: regions of one chromosome
MAX_TABLE = 1 << 24              # csrc/aggregate.hip AGG_MAX_TABLE: G P P K entries of either table
COORD_LIMIT = 1 << 30            # csrc/interval_lists.h COORD_LIMIT: |c| of a feature's coordinate stays below it


def _check_features(features):
    """-> int64 [N, 7]: chrom, a0, a1, b0, b1, group, flip"""
    f = np.asarray(features)
    if f.size == 0:
        return np.zeros((0, 7), dtype=np.int64)
    if f.ndim != 2 or f.shape[1] != 7 or f.dtype.kind not in "iu":
        raise ValueError("features must be an integer array of rows chrom, a0, a1, b0, b1, group, flip (got %s %s)" % (f.dtype, f.shape))
    f = f.astype(np.int64)
    if np.any(f[:, 2] <= f[:, 1]) or np.any(f[:, 4] <= f[:, 3]):
        raise ValueError("a feature's intervals are half-open [a0, a1) and [b0, b1) of at least one bin: a1 > a0 and b1 > b0")
    if np.abs(f[:, 1:5]).max() >= COORD_LIMIT:
        raise ValueError("a feature's bins must stay below 2^30")
    if f[:, 5].min() < 0:
        raise ValueError("a feature's group must be >= 0")
    if f[:, 6].min() < 0 or f[:, 6].max() > 1:
        raise ValueError("a feature's flip must be 0 or 1")
    return f


def _check_grid(body, flank):
    T, F = int(body), int(flank)
    if T < 1 or T > MAX_BODY:
        raise ValueError("body must be in 1 .. %d cells" % MAX_BODY)
    if F < 0 or F > MAX_FLANK:
        raise ValueError("flank must be in 0 .. %d cells" % MAX_FLANK)
    return T, F


def axis_cells(x0, x1, T, F):
    """-> (lo, hi), int64 [T + 2 F] each: cell c of the interval [x0, x1) holds the bins [lo[c], hi[c]).  Host only."""
    x0, x1, T, F = int(x0), int(x1), int(T), int(F)
    if x1 <= x0 or T < 1 or F < 0:
        raise ValueError("axis_cells takes an interval of at least one bin, T >= 1 and F >= 0")
    edge = x0 + (np.arange(-F, T + F + 1, dtype=np.int64) * (x1 - x0)) // T       # (NumPy's // is the floor)
    return edge[:-1].copy(), np.maximum(edge[:-1] + 1, edge[1:])


def is_small(na, nb, T):
    """whether a feature of na x nb bins goes through the kernel of a lane per pile cell: ceil(na / T) ceil(nb / T) <= SMALL_AREA"""
    return (-(-int(na) // int(T))) * (-(-int(nb) // int(T))) <= SMALL_AREA


def state_aggregate(state_vec, len_vec, features, body, flank, K=None, G=None):
    """features int64 [N, 7] of rows chrom, a0, a1, b0, b1, group, flip in chromosome bins -> dict:
      cells int64 [G, P, P, K]       the bin pairs of state k in pile cell (u, v), summed over the features of group g
      votes int64 [G, P, P, K]       the features of group g whose pile cell (u, v) is not empty and mostly k (lowest k on ties)
      n_features int64 [G]           the features given per group
      features_chrom                 int64 [C, 2] of rows chrom, the features submitted for it: the chromosomes of len_vec
      K, G, body, flank
    The map is uploaded once; every chromosome that has both features and regions gets one phmrf_state_aggregate call with
    all of its regions, and the calls' tables are summed.  Features are not deduplicated.  K: the largest state + 1 by
    default, G: the largest group + 1; a state >= K inside some cell is an error (RuntimeError), outside every cell it is not
    looked at.  RuntimeError without a GPU."""
    from . import _lib
    import torch
    s = check_state_vec(state_vec)
    L = check_len_vec(len_vec, s.shape[0])
    T, F = _check_grid(body, flank)
    f = _check_features(features)
    K = check_K(s, K)
    G = check_G(f[:, 5], G)
    if f.shape[0] and f[:, 5].max() >= G:
        raise ValueError("a feature's group must be below G = %d" % G)
    P = T + 2 * F
    if G * P * P * K > MAX_TABLE:
        raise ValueError("G (body + 2 flank)^2 K = %d entries is above %d" % (G * P * P * K, MAX_TABLE))
    lib, dev, stream = device()
    cells = np.zeros((G, P, P, K), dtype=np.int64)
    votes = np.zeros_like(cells)
    chroms = np.unique(L[:, 9])
    features_chrom = np.stack([chroms, np.zeros_like(chroms)], axis=1)
    s_t = torch.from_numpy(s.astype(np.uint8)).to(dev) if s.size else None
    for t, chrom in enumerate(chroms):
        sel = f[f[:, 0] == chrom]
        rows = L[L[:, 9] == chrom]
        if not sel.shape[0] or s_t is None:
            continue
        if rows.shape[0] > MAX_REGIONS:
            raise ValueError("chromosome %d has %d regions, above %d" % (chrom, rows.shape[0], MAX_REGIONS))
        sel = sel[np.argsort(sel[:, 5], kind="stable")]
        offsets = np.concatenate([[0], np.cumsum(np.bincount(sel[:, 5], minlength=G))]).astype(np.int64)
        regs = np.ascontiguousarray(rows[:, [1, 3, 4, 5, 6, 8]], dtype=np.int64)
        feat_t = torch.from_numpy(np.ascontiguousarray(sel[:, 1:5], dtype=np.int32)).to(dev)
        flip_t = torch.from_numpy(np.ascontiguousarray(sel[:, 6], dtype=np.uint8)).to(dev)
        part_c, part_v = np.zeros_like(cells), np.zeros_like(cells)
        _lib.check(lib.phmrf_state_aggregate(ctypes.c_void_p(s_t.data_ptr()), s.shape[0], regs.shape[0], _lib.ptr_i64(regs), K, T, F, G,
                                             _lib.ptr_i64(offsets), ctypes.c_void_p(feat_t.data_ptr()), ctypes.c_void_p(flip_t.data_ptr()),
                                             _lib.ptr_i64(part_c), _lib.ptr_i64(part_v), stream))
        features_chrom[t, 1] = sel.shape[0]
        cells += part_c
        votes += part_v
    return dict(cells=cells, votes=votes, n_features=np.bincount(f[:, 5], minlength=G).astype(np.int64), features_chrom=features_chrom,
                K=np.int64(K), G=np.int64(G), body=np.int64(T), flank=np.int64(F))


# ---- the feature files ------------------------------------------------------------------------------------------------------
def _read(rows, names, skipped, short):
    return dict(features=np.array(rows, dtype=np.int64).reshape(-1, 7), names=names, skipped_lines=skipped, skipped_short=short)


def read_features(path, len_vec, resolution, min_bp=0):
    """A BED file `chrom start stop [name [score [strand]]]` (tabs or spaces; lines that start with # and blank lines are
    skipped) -> dict:
      features int64 [N, 7]   chrom, a0, a1, a0, a1, group, flip: A = B, the bins the interval OVERLAPS (query's bin rule:
                              a0 = start // resolution, a1 = max(a0 + 1, ceil(stop / resolution)))
      names                   the distinct names in order of first appearance (a line without one is named `feature`): group g
                              is names[g]; at most 8
      skipped_lines           the lines of chromosomes len_vec does not hold
      skipped_short           the lines of held chromosomes with stop - start < min_bp
    chrom is chr<N> or <N>, N the integer in len_vec's column 9.  Strand - sets flip (the pile is read against the genome's
    direction); +, . and no strand do not.  The names are numbered over the whole file.  ValueError for a malformed line,
    stop < start, a negative coordinate, any other strand and a ninth name.  Host only."""
    res, min_bp, held = check_resolution(resolution), int(min_bp), held_chroms(len_vec)
    rows, names, skipped, short = [], [], 0, 0
    for number, _, chroms, ((start, stop),), rest in interval_lines(path, 1, "chrom start stop [name [score [strand]]]", True):
        a0, a1 = overlap_bins(start, stop, res)
        strand = rest[2] if len(rest) > 2 else "."
        if strand not in ("+", "-", "."):
            raise ValueError("%s line %d: strand %r is not +, - or ." % (path, number, strand))
        g = name_group(path, number, names, rest[0] if rest else "feature")
        c = held_chrom(chroms, held)
        if c is None:
            skipped += 1
        elif stop - start < min_bp:
            short += 1
        else:
            rows.append([c, a0, a1, a0, a1, g, 1 if strand == "-" else 0])
    return _read(rows, names, skipped, short)


def read_feature_pairs(path, len_vec, resolution, min_bp=0):
    """A BEDPE file `chrom1 start1 stop1 chrom2 start2 stop2 [name]` -> read_features' dict with the features chrom, a0, a1,
    b0, b1, group, 0: A and B the bins the two intervals overlap, swapped so that a0 <= b0 (the pile's u axis is the end
    nearer the chromosome's start, as in --pileup).  A line whose two ends are not on one chromosome of len_vec is skipped
    and counted, a line with an end shorter than min_bp too; a line without a name is named `pair`.  Host only."""
    res, min_bp, held = check_resolution(resolution), int(min_bp), held_chroms(len_vec)
    rows, names, skipped, short = [], [], 0, 0
    for number, _, chroms, spans, rest in interval_lines(path, 2, "chrom1 start1 stop1 chrom2 start2 stop2 [name]", True):
        (a0, a1), (b0, b1) = (overlap_bins(start, stop, res) for start, stop in spans)
        g = name_group(path, number, names, rest[0] if rest else "pair")
        c = held_chrom(chroms, held)
        if c is None:
            skipped += 1
        elif min(stop - start for start, stop in spans) < min_bp:
            short += 1
        else:
            rows.append([c] + ([a0, a1, b0, b1] if a0 <= b0 else [b0, b1, a0, a1]) + [g, 0])
    return _read(rows, names, skipped, short)


def with_controls(features, shift_bins, G):
    """-> the features and, behind them, for every feature of group g the two features moved by -shift and by +shift bins
    ALONG the diagonal (both intervals move together, so every bin pair keeps its genomic distance: query.with_controls'
    rule) as group G + g with the same flip.  A control with a negative bin is dropped.  Host only."""
    f = _check_features(features)
    ctl, keep = shift_along_diagonal(f, ((1, 2), (3, 4)), shift_bins)
    G = int(G)
    if G < 1 or (f.shape[0] and f[:, 5].max() >= G):
        raise ValueError("G must be >= 1 and above every feature's group")
    ctl[:, 5] += G
    return np.concatenate([f, ctl[keep]])


# ---- reading and writing a pile ---------------------------------------------------------------------------------------------
def aggregate_lines(votes, cells, names, body, flank, ctl_votes=None):
    """-> the lines of aggregate_*.txt, header first: per name and pile cell the name, u and v as cell indices and as
    positions in feature lengths ((u - F + 0.5) / T: 0 .. 1 is the body), the features voting, the dominant state + 1 by
    votes (0 for an empty cell), its vote share, the entropy of the votes in bits, the bin pairs of `cells`, with controls
    their votes and the log2 ratio of the dominant state's vote share, then the K vote counts"""
    o, c = np.asarray(votes), np.asarray(cells)
    G, P, _, K = o.shape
    T, F = int(body), int(flank)
    pairs = c.sum(axis=-1)
    (core_head, tail_head), fields = summary_fields(o, ctl_votes, "control_features")
    lines = ["\t".join(["#name", "u", "v", "u_pos", "v_pos", "features"] + core_head + ["bin_pairs"] + tail_head) + "\n"]
    for g in range(G):
        for a in range(P):
            for b in range(P):
                core, tail = fields((g, a, b))
                f = [names[g], "%d" % a, "%d" % b, "%.4f" % ((a - F + 0.5) / T), "%.4f" % ((b - F + 0.5) / T)]
                lines.append("\t".join(f + core + ["%d" % pairs[g, a, b]] + tail) + "\n")
    return lines


def aggregate_files(path, output_path, resolution, field="state_vec", bed="", bedpe="", body=32, flank=16, shift_bp=0, min_bp=0,
                    palette_path=""):
    """The command line's --aggregate: pile the `field` of one estimate_ou_*.mat / segment_*.mat / smooth_*.mat up over the
    features of `bed` (read_features) or the interval pairs of `bedpe` (read_feature_pairs) on a grid of `body` + 2 `flank`
    cells, with controls at shift_bp when it is not 0.  Writes under output_path aggregate_<stem>.npz (cells and votes [G, P,
    P, K] of the names' groups, with a shift ctl_cells, ctl_votes and log2_ratio on the votes, n_features and features_chrom
    over the groups and their controls, names, skipped_lines, skipped_short, body, flank, shift in bins, K, len_vec, palette
    and the settings; no pickles), aggregate_<stem>.txt (aggregate_lines) and one aggregate_<stem>_<name>.png per name
    (pileup.pile_image of the votes: the dominant state by votes at 8 x 8 pixels a cell).  -> the .npz"""
    res = check_resolution(resolution)
    if bool(bed) == bool(bedpe):
        raise ValueError("aggregate_files takes a bed file or a bedpe file, one of the two")
    T, F = _check_grid(body, flank)
    shift = check_shift(res, shift_bp)
    if int(min_bp) < 0:
        raise ValueError("min_bp must be >= 0")
    s, L, _ = load_map(path, field)
    read = read_features(bed, L, res, min_bp) if bed else read_feature_pairs(bedpe, L, res, min_bp)
    names = read["names"] or ["feature" if bed else "pair"]
    G, K = len(names), (int(s.max()) + 1 if s.size else 1)
    features = with_controls(read["features"], shift, G) if shift else read["features"]
    result = state_aggregate(s, L, features, T, F, K=K, G=2 * G if shift else G)
    cells, votes = result["cells"][:G], result["votes"][:G]
    extra, ctl_votes = {}, None
    if shift:
        ctl_votes = result["votes"][G:]
        extra = dict(ctl_cells=result["cells"][G:], ctl_votes=ctl_votes, log2_ratio=log2_ratio(votes, ctl_votes))
    palette = load_palette(palette_path, K) if palette_path else default_palette(K)
    os.makedirs(output_path, exist_ok=True)
    name = stem(path)
    out = os.path.join(output_path, "aggregate_%s.npz" % name)
    np.savez(out, cells=cells, votes=votes, n_features=result["n_features"], features_chrom=result["features_chrom"],
             names=np.array(names), skipped_lines=np.int64(read["skipped_lines"]), skipped_short=np.int64(read["skipped_short"]),
             body=np.int64(T), flank=np.int64(F), shift=np.int64(shift), K=np.int64(K), len_vec=L, palette=palette,
             resolution=np.int64(res), aggregate_field=np.array(field), features_file=np.array(os.path.basename(bed or bedpe)),
             feature_kind=np.array("bed" if bed else "bedpe"), shift_bp=np.int64(shift_bp), min_bp=np.int64(min_bp), **extra)
    with open(os.path.join(output_path, "aggregate_%s.txt" % name), "wb") as fh:
        fh.write("".join(aggregate_lines(votes, cells, names, T, F, ctl_votes)).encode())
    write_group_images(output_path, "aggregate_%s" % name, names, [pile_image(votes[g], palette) for g in range(G)])
    return out
