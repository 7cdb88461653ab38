"""Pile a state map up around genomic anchors: what does the map look like AROUND my features -- the
state composition across TAD boundaries, at and beside CTCF sites oriented by strand, in the corner where two loop anchors
meet.  A centre is a bin pair (a, b) of one chromosome with a group and an orientation; a pile cell (u, v) with u, v in
[-w, w] reads the cell (a + s p, b + s q) of the chromosome's symmetric matrix, (p, q) = (v, u) when the centre is transposed
(orient bit 1) else (u, v), s = -1 when it is flipped (orient bit 0) else +1.

`state_pileup(state_vec, len_vec, centres, flank, K=None, G=None)` counts on the GPU, region by region
(phmrf_state_pileup, csrc/pileup.hip), obs[g][u + w][v + w][k] = the centres of group g whose pile cell (u, v) lies on a cell
in state k, and sums over the regions.  `read_anchors(...)` reads a BED file into on-diagonal centres, `read_anchor_pairs(...)`
a BEDPE file into centres off it, `with_controls(...)` adds centres shifted ALONG the diagonal (the same genomic distance:
the project's rule for an expectation), `pile_summary(...)` and `log2_ratio(...)` read a pile on the host,
`pileup_files(...)` is the command line's --pileup FILE.mat.

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

from .intervals import (MAX_GROUPS, MAX_NAMES, check_G, check_shift, held_chrom, held_chroms, interval_lines, log2_ratio, name_group,
                        pile_summary, shift_along_diagonal, summary_fields, write_group_images)
from .maps import check_K, check_len_vec, check_state_vec, device, load_map, regions, stem
from .maps import check_resolution as _resolution
from .render import default_palette, load_palette

LANES = 256                      # csrc/pileup.hip PILEUP_LANES: pile cells of a tile = lanes of a workgroup
CHUNK = 256                      # csrc/pileup.hip PILEUP_CHUNK: centres of one group a workgroup piles at a time
GRID_CAP = 4096                  # csrc/pileup.hip PILEUP_GRID_CAP: workgroups
MAX_FLANK = 64                   # csrc/pileup.hip PILEUP_MAX_FLANK: w <= 64 bins on either side of a centre
FLIP, TRANSPOSE = 1, 2           # the bits of an orient
PIXELS = 8                       # side of a pile cell in pileup_*.png


def _check_centres(centres):
    """-> int64 [N, 5]: chrom, bin_a, bin_b, group, orient"""
    c = np.asarray(centres)
    if c.size == 0:
        return np.zeros((0, 5), dtype=np.int64)
    if c.ndim != 2 or c.shape[1] != 5 or c.dtype.kind not in "iu":
        raise ValueError("centres must be an integer array of rows chrom, bin_a, bin_b, group, orient (got %s %s)" % (c.dtype, c.shape))
    c = c.astype(np.int64)
    if c[:, 3].min() < 0:
        raise ValueError("a centre's group must be >= 0")
    if c[:, 4].min() < 0 or c[:, 4].max() > 3:
        raise ValueError("a centre's orient must be in 0 .. 3 (bit 0: flip, bit 1: transpose)")
    return c


def _check_flank(flank):
    w = int(flank)
    if w < 0 or w > MAX_FLANK:
        raise ValueError("flank must be in 0 .. %d bins" % MAX_FLANK)
    return w


def region_centres(centres, row, w, G):
    """What one region (a row of len_vec) is given of checked centres [N, 5]: the centres of its chromosome in its local
    coordinates, for an off-diagonal region their mirror images with orient ^ 2 too, without those whose window of +- w
    cannot touch the region, in the order of their groups -> (offsets int64 [G + 1], ci int32, cj int32, orient u8), the
    arguments of phmrf_state_pileup.  Host only."""
    H, W, s1, s2, diag = (int(row[x]) for x in (3, 4, 5, 6, 8))
    sel = centres[centres[:, 0] == row[9]]
    ci, cj, grp, ori = sel[:, 1] - s1, sel[:, 2] - s2, sel[:, 3], sel[:, 4]
    if not diag:
        ci, cj = np.concatenate([ci, sel[:, 2] - s1]), np.concatenate([cj, sel[:, 1] - s2])
        grp, ori = np.concatenate([grp, grp]), np.concatenate([ori, ori ^ TRANSPOSE])
    keep = (ci + w >= 0) & (ci - w < H) & (cj + w >= 0) & (cj - w < W)
    order = np.argsort(grp[keep], kind="stable")
    ci, cj, grp, ori = (x[keep][order] for x in (ci, cj, grp, ori))
    offsets = np.concatenate([[0], np.cumsum(np.bincount(grp, minlength=G))]).astype(np.int64)
    return offsets, ci.astype(np.int32), cj.astype(np.int32), ori.astype(np.uint8)


def state_pileup(state_vec, len_vec, centres, flank, K=None, G=None):
    """centres int64 [N, 5] of rows chrom, bin_a, bin_b, group, orient in chromosome bins -> dict:
      obs int64 [G, 2w + 1, 2w + 1, K]   the centres of group g whose pile cell (u, v) lies on a cell in state k, all regions
      centres_region int64 [R, G]        the centres submitted to each region, after the windows that cannot touch it are left out
      n_centres int64 [G]                the centres given per group
      K, G, flank
    Every region of the centre's chromosome gets the centre at the local (bin_a - start_bin1, bin_b - start_bin2); an
    off-diagonal region also its mirror image (bin_b - start_bin1, bin_a - start_bin2) with orient ^ 2, a diagonal region is
    mirrored by the entry point.  So every cell of the chromosome's symmetric matrix that a region covers counts exactly
    once (regions that overlap each other, or their own mirror image, count where they overlap once each); cells that no
    region covers are not counted.  Centres are not deduplicated.  K: the largest state + 1 by default, G: the largest
    group + 1; a state >= K inside a window is an error, outside every window it is not looked at."""
    from . import _lib
    import torch
    s = check_state_vec(state_vec)
    L = check_len_vec(len_vec, s.shape[0])
    w = _check_flank(flank)
    c = _check_centres(centres)
    K = check_K(s, K)
    G = check_G(c[:, 3], G)
    if c.shape[0] and c[:, 3].max() >= G:
        raise ValueError("a centre's group must be below G = %d" % G)
    lib, dev, stream = device()
    side = 2 * w + 1
    obs = np.zeros((G, side, side, K), dtype=np.int64)
    centres_region = np.zeros((L.shape[0], G), dtype=np.int64)
    s_t = torch.from_numpy(s.astype(np.uint8)).to(dev)
    for r, lo, hi, H, W, diag, _ in regions(L):
        offsets, ci, cj, ori = region_centres(c, L[r], w, G)
        if not offsets[G]:
            continue
        centres_region[r] = np.diff(offsets)
        ci_t, cj_t, ori_t = (torch.from_numpy(x).to(dev) for x in (ci, cj, ori))
        part = np.zeros_like(obs)
        _lib.check(lib.phmrf_state_pileup(ctypes.c_void_p(s_t[lo:hi].data_ptr()), H, W, diag, K, w, G, _lib.ptr_i64(offsets),
                                          ctypes.c_void_p(ci_t.data_ptr()), ctypes.c_void_p(cj_t.data_ptr()),
                                          ctypes.c_void_p(ori_t.data_ptr()), _lib.ptr_i64(part), stream))
        obs += part
    return dict(obs=obs, centres_region=centres_region, n_centres=np.bincount(c[:, 3], minlength=G).astype(np.int64),
                K=np.int64(K), G=np.int64(G), flank=np.int64(w))


# ---- the anchor files -------------------------------------------------------------------------------------------------------
def _anchors(rows, names, skipped):
    return dict(centres=np.array(rows, dtype=np.int64).reshape(-1, 5), names=names, skipped_lines=skipped)


def read_anchors(path, len_vec, resolution):
    """A BED file `chrom start stop [name [score [strand]]]` (tabs or spaces; lines that start with # and blank lines are
    skipped) -> dict:
      centres int64 [N, 5]   chrom, a, a, group, orient: the anchor's bin a = ((start + stop) // 2) // resolution on the diagonal
      names                  the distinct names in order of first appearance (a line without one is named `anchor`): group g
                             is names[g]; at most 8
      skipped_lines          the lines of chromosomes len_vec does not hold
    chrom is chr<N> or <N>, N the integer in len_vec's column 9.  Strand - gives orient 1 (flip: the pile is read against the
    genome's direction); +, . and no strand give 0.  The names are numbered over the whole file.  ValueError for a malformed
    line, start >= stop, a negative coordinate, any other strand and a ninth name.  Host only."""
    res, held = _resolution(resolution), held_chroms(len_vec)
    rows, names, skipped = [], [], 0
    for number, _, chroms, ((start, stop),), rest in interval_lines(path, 1, "chrom start stop [name [score [strand]]]", False):
        mid = (start + stop) // 2
        strand = rest[2] if len(rest) > 2 else "."
        if strand not in ("+", "-", "."):
            raise ValueError("%s line %d: strand %r is not +, - or ." % (path, number, strand))
        g = name_group(path, number, names, rest[0] if rest else "anchor")
        c = held_chrom(chroms, held)
        if c is None:
            skipped += 1
            continue
        rows.append([c, mid // res, mid // res, g, FLIP if strand == "-" else 0])
    return _anchors(rows, names, skipped)


def read_anchor_pairs(path, len_vec, resolution):
    """A BEDPE file `chrom1 start1 stop1 chrom2 start2 stop2 [name]` -> read_anchors' dict with the centres chrom, a, b, group,
    0: a <= b the bins of the two intervals' midpoints.  A line whose two ends are not on one chromosome of len_vec is
    skipped and counted; a line without a name is named `pair`.  Host only."""
    res, held = _resolution(resolution), held_chroms(len_vec)
    rows, names, skipped = [], [], 0
    for number, _, chroms, spans, rest in interval_lines(path, 2, "chrom1 start1 stop1 chrom2 start2 stop2 [name]", False):
        a, b = ((start + stop) // 2 // res for start, stop in spans)
        g = name_group(path, number, names, rest[0] if rest else "pair")
        c = held_chrom(chroms, held)
        if c is None:
            skipped += 1
            continue
        rows.append([c, min(a, b), max(a, b), g, 0])
    return _anchors(rows, names, skipped)


def with_controls(centres, shift_bins, G):
    """-> the centres and, behind them, for every centre (a, b) of group g the controls (a - shift, b - shift) and
    (a + shift, b + shift) of group G + g with the same orient: shifted ALONG the diagonal, so at the centre's own genomic
    distance.  A control with a negative bin is dropped.  Host only."""
    c = _check_centres(centres)
    ctl, keep = shift_along_diagonal(c, ((1,), (2,)), shift_bins)
    G = int(G)
    if G < 1 or (c.shape[0] and c[:, 3].max() >= G):
        raise ValueError("G must be >= 1 and above every centre's group")
    ctl[:, 3] += G
    return np.concatenate([c, ctl[keep]])


# ---- reading a pile ---------------------------------------------------------------------------------------------------------
def pileup_lines(obs, names, flank, resolution, ctl=None):
    """-> the lines of pileup_*.txt, header first: per group and pile cell the name, u and v in bp, the total, the dominant
    state + 1 (0 for an empty cell), its share, the entropy in bits, with a control the control's total and the log2 ratio of
    the dominant state, then the K counts"""
    o = np.asarray(obs)
    G, side, _, K = o.shape
    w, res = int(flank), int(resolution)
    (core_head, tail_head), fields = summary_fields(o, ctl)
    lines = ["\t".join(["#name", "u_bp", "v_bp", "total"] + core_head + tail_head) + "\n"]
    for g in range(G):
        for a in range(side):
            for b in range(side):
                core, tail = fields((g, a, b))
                lines.append("\t".join([names[g], "%d" % ((a - w) * res), "%d" % ((b - w) * res)] + core + tail) + "\n")
    return lines


def pile_image(obs_g, palette):
    """obs_g [side, side, K] of one group -> u8 [8 side, 8 side, 3]: every pile cell a square in its dominant state's colour,
    white when empty; u runs down, v to the right"""
    dom = pile_summary(obs_g)["dominant"]
    rgb = np.where((dom >= 0)[..., None], np.asarray(palette)[np.maximum(dom, 0)], 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(rgb, PIXELS, axis=0), PIXELS, axis=1))


def check_bins(resolution, flank_bp, shift_bp):
    """-> (w, shift) in bins: w = flank_bp // resolution in 0 .. 64; a shift is a whole number of bins (0: no controls)"""
    res, flank_bp = _resolution(resolution), int(flank_bp)
    if flank_bp < 0 or flank_bp // res > MAX_FLANK:
        raise ValueError("the flank must be 0 .. %d bins of %d bp, not %d bp" % (MAX_FLANK, res, flank_bp))
    return flank_bp // res, check_shift(res, shift_bp)


def pileup_files(path, output_path, resolution, field="state_vec", bed="", bedpe="", flank_bp=1000000, shift_bp=0, palette_path=""):
    """The command line's --pileup: pile the `field` of one estimate_ou_*.mat / segment_*.mat / smooth_*.mat up around the
    anchors of `bed` (read_anchors) or the anchor pairs of `bedpe` (read_anchor_pairs), with controls at shift_bp when it is
    not 0.  Writes under output_path pileup_<stem>.npz (obs [G, ...] of the names' groups, ctl [G, ...] of their controls
    when there is a shift, log2_ratio (all NaN without a shift), n_centres and centres_region over the groups and their
    controls, names, skipped_lines, flank and shift in bins, K, len_vec and the settings; no pickles), pileup_<stem>.txt
    (pileup_lines) and one pileup_<stem>_<name>.png per group (pile_image).  -> the .npz"""
    res = _resolution(resolution)
    if bool(bed) == bool(bedpe):
        raise ValueError("pileup_files takes a bed file or a bedpe file, one of the two")
    w, shift = check_bins(res, flank_bp, shift_bp)
    s, L, _ = load_map(path, field)
    anchors = read_anchors(bed, L, res) if bed else read_anchor_pairs(bedpe, L, res)
    names = anchors["names"] or ["anchor" if bed else "pair"]
    G, K = len(names), (int(s.max()) + 1 if s.size else 1)
    centres = with_controls(anchors["centres"], shift, G) if shift else anchors["centres"]
    result = state_pileup(s, L, centres, w, K=K, G=2 * G if shift else G)
    obs = result["obs"][:G]
    ctl = result["obs"][G:] if shift else None
    palette = load_palette(palette_path, K) if palette_path else default_palette(K)
    os.makedirs(output_path, exist_ok=True)
    name = stem(path)
    out = os.path.join(output_path, "pileup_%s.npz" % name)
    extra = {} if ctl is None else dict(ctl=ctl)
    np.savez(out, obs=obs, n_centres=result["n_centres"], centres_region=result["centres_region"],
             log2_ratio=log2_ratio(obs, np.zeros_like(obs) if ctl is None else ctl), names=np.array(names),
             skipped_lines=np.int64(anchors["skipped_lines"]), flank=np.int64(w), shift=np.int64(shift), K=np.int64(K), len_vec=L,
             resolution=np.int64(res), pileup_field=np.array(field), anchors=np.array(os.path.basename(bed or bedpe)),
             anchor_kind=np.array("bed" if bed else "bedpe"), flank_bp=np.int64(flank_bp), shift_bp=np.int64(shift_bp),
             palette=palette, **extra)
    with open(os.path.join(output_path, "pileup_%s.txt" % name), "wb") as fh:
        fh.write("".join(pileup_lines(obs, names, w, res, ctl)).encode())
    write_group_images(output_path, "pileup_%s" % name, names, [pile_image(obs[g], palette) for g in range(G)])
    return out
