"""What the modes that read a LIST of genomic intervals share (pileup, query, aggregate; enrich reads its annotation through
the same parser): the lines of a BED / BEDPE file with their refusals, the bin rule, the numbering of names into groups, the
chromosomes a len_vec holds, controls shifted along the diagonal, the checks of a group count and a shift, the summary of a
table of counts with the columns every *_lines writer shares, and the loop that writes one image per group.  Host only.
"""
import os
import re

import numpy as np

from .maps import annotation_lines, chrom_of, is_number
from .render import write_png

MAX_GROUPS = 16                  # csrc/interval_lists.h MAX_GROUPS: 8 names and their 8 controls
MAX_NAMES = 8


# ---- the interval files -----------------------------------------------------------------------------------------------------
def interval_lines(path, ends, expected, empty_ok, fields=None):
    """The lines of a BED (ends = 1) or BEDPE (ends = 2) file `chrom start stop` [x ends] ... -> yields (line number, the line,
    the chromosome(s) as written, the (start, stop) of every end in bp, the fields behind them).  ValueError for a line of
    fewer than `fields` fields (3 ends by default) or with a coordinate that is no integer (`expected` is the format the
    message names), for a negative coordinate, and for start >= stop -- with empty_ok only for stop < start: a zero-length
    interval is let through."""
    need = 3 * ends
    for number, line, f in annotation_lines(path):
        if len(f) < (fields or need) or not all(is_number(f[3 * e + t]) for e in range(ends) for t in (1, 2)):
            raise ValueError("%s line %d: expected `%s`, got %r" % (path, number, expected, line))
        spans = []
        for e in range(ends):
            start, stop = int(f[3 * e + 1]), int(f[3 * e + 2])
            if start < 0 or stop < 0:
                raise ValueError("%s line %d: negative coordinate" % (path, number))
            if empty_ok and stop < start:
                raise ValueError("%s line %d: stop %d < start %d" % (path, number, stop, start))
            if not empty_ok and start >= stop:
                raise ValueError("%s line %d: start %d >= stop %d" % (path, number, start, stop))
            spans.append((start, stop))
        yield number, line, f[0:need:3], spans, f[need:]


def overlap_bins(start, stop, res):
    """THE BIN RULE of --query and --aggregate -> (a0, a1): the bins [a0, a1) that [start, stop) bp overlaps, at least one"""
    a0 = start // res
    return a0, max(a0 + 1, -(-stop // res))


def name_group(path, number, names, name, limit=MAX_NAMES, why=""):
    """-> the index of `name` in `names`, appended when it is new; ValueError for more than `limit` names"""
    if name not in names:
        if len(names) == limit:
            raise ValueError("%s line %d: more than %d names (%s, then %r)%s" % (path, number, limit, ", ".join(names), name, why))
        names.append(name)
    return names.index(name)


def held_chroms(len_vec):
    """-> the set of the chromosomes of len_vec (column 9)"""
    return set(int(c) for c in np.unique(np.asarray(len_vec)[:, 9]))


def held_chrom(chroms, held):
    """-> the number of the one chromosome all of `chroms` (as written) name when `held` has it, else None: the line is skipped"""
    c = chrom_of(chroms[0])
    return c if c in held and all(chrom_of(x) == c for x in chroms[1:]) else None


# ---- groups, shifts and controls --------------------------------------------------------------------------------------------
def check_G(groups, G):
    """-> G: the largest of `groups` + 1 by default (1 without any), in 1 .. MAX_GROUPS"""
    G = (int(groups.max()) + 1 if groups.shape[0] else 1) if G is None else int(G)
    if G < 1 or G > MAX_GROUPS:
        raise ValueError("G must be in 1 .. %d" % MAX_GROUPS)
    return G


def check_shift(res, shift_bp):
    """-> the shift in bins of `res` bp: a whole number of them (0: no controls)"""
    shift_bp = int(shift_bp)
    if shift_bp < 0 or shift_bp % res:
        raise ValueError("the shift must be a whole number of bins of %d bp (0: no controls), not %d bp" % (res, shift_bp))
    return shift_bp // res


def shift_along_diagonal(rows, columns, shift):
    """rows int64 [N, C]; columns: per interval of a row its bin columns -> (int64 [2 N, C], keep bool [2 N]): per row the copy
    with every bin column moved by -shift, then the copy moved by +shift (ALONG the diagonal: all intervals move together, so
    every bin pair keeps its genomic distance); keep: the first column of every interval is still >= 0."""
    shift = int(shift)
    if shift < 1:
        raise ValueError("shift_bins must be >= 1")
    moved = [c for interval in columns for c in interval]
    both = np.stack([rows, rows], axis=1)                     # per row: the control before it, the control after it
    both[:, 0, moved] -= shift
    both[:, 1, moved] += shift
    ctl = both.reshape(-1, rows.shape[1])
    return ctl, np.all(ctl[:, [interval[0] for interval in columns]] >= 0, axis=1)


# ---- reading and writing a table of counts ----------------------------------------------------------------------------------
def pile_summary(obs):
    """obs [..., K] -> dict over the pile cells: total int64, dominant int64 (the state with the largest count, the lowest on
    ties, -1 for an empty cell), share float64 (the dominant state's; 0 for an empty cell), entropy float64 in bits (0 for
    an empty cell).  Host only."""
    o = np.asarray(obs).astype(np.int64)
    total = o.sum(axis=-1)
    full = total > 0
    dominant = np.where(full, np.argmax(o, axis=-1), -1)
    p = np.divide(o, total[..., None], out=np.zeros(o.shape), where=full[..., None])
    logp = np.zeros(o.shape)
    np.log2(p, out=logp, where=p > 0)
    return dict(total=total, dominant=dominant, share=p.max(axis=-1) if o.shape[-1] else np.zeros(total.shape),
                entropy=np.abs((p * logp).sum(axis=-1)))


def log2_ratio(obs, ctl):
    """-> log2(share_obs / share_ctl + 1e-16) per pile cell and state, share = count / the cell's total; NaN where either
    total is 0 or the control's share is 0.  Host only."""
    o, c = np.asarray(obs, dtype=np.float64), np.asarray(ctl, dtype=np.float64)
    if o.shape != c.shape:
        raise ValueError("log2_ratio takes two piles of one shape (got %s and %s)" % (o.shape, c.shape))
    to, tc = o.sum(axis=-1, keepdims=True), c.sum(axis=-1, keepdims=True)
    ok = (to > 0) & (tc > 0) & (c > 0)
    share_o = np.divide(o, to, out=np.zeros(o.shape), where=ok)
    share_c = np.divide(c, tc, out=np.ones(o.shape), where=ok)
    ratio = np.divide(share_o, share_c, out=np.zeros(o.shape), where=ok)
    out = np.full(o.shape, np.nan)
    np.log2(ratio + 1e-16, out=out, where=ok)
    return out


def summary_fields(counts, ctl=None, control="control_total"):
    """counts [..., K], ctl of the same shape or None -> (head, fields): what the lines of pileup_*.txt, query_*.txt and
    aggregate_*.txt share.  head = (the core's column names, the tail's); fields(at) for the index tuple `at` of a cell ->
    (core, tail): core = the total, the dominant state + 1 (0 for an empty cell), its share, the entropy in bits; tail =
    with ctl the control's total (the column `control`) and the log2 ratio of the dominant state, then the K counts."""
    o = np.asarray(counts)
    sm = pile_summary(o)
    if ctl is not None:
        ctl_total, l2 = np.asarray(ctl).sum(axis=-1), log2_ratio(o, ctl)
    head = (["dominant_state", "share", "entropy_bits"], ([] if ctl is None else [control, "log2_ratio"])
            + ["state_%d" % (k + 1) for k in range(o.shape[-1])])

    def fields(at):
        dom = int(sm["dominant"][at])
        core = ["%d" % sm["total"][at], "%d" % (dom + 1), "%.6f" % sm["share"][at], "%.6f" % sm["entropy"][at]]
        tail = [] if ctl is None else ["%d" % ctl_total[at], "%.4f" % (l2[at + (dom,)] if dom >= 0 else np.nan)]
        return core, tail + ["%d" % x for x in o[at]]

    return head, fields


def write_group_images(output_path, prefix, names, images):
    """writes images[g] (u8 [h, w, 3]) to output_path/<prefix>_<name g>.png, the name with every character outside
    A-Za-z0-9._- replaced by _ and, where that repeats an earlier file's, _g<g> behind it"""
    used = set()
    for g, group in enumerate(names):
        safe = re.sub(r"[^A-Za-z0-9._-]", "_", group)
        if safe in used:
            safe = "%s_g%d" % (safe, g)
        used.add(safe)
        write_png(os.path.join(output_path, "%s_%s.png" % (prefix, safe)), images[g])
