"""1-D genome tracks of ONE state map: the state composition of every genomic bin's row of the contact
matrix, optionally restricted to a window of genomic distance -- what a genome browser shows beside TAD boundaries,
compartments or replication timing (the reference's utility.py gestures at it with intersect_region and write_tobed).

`state_tracks(state_vec, len_vec, windows=((0, -1),), K=None)` counts, region by region and window by window, the states of
every row and every column of the region's full matrix on the GPU (phmrf_state_tracks, csrc/tracks.hip) and merges the
regions of a chromosome into one track along the genome.  `track_summary(track)` reads a track per bin (host only):
dominant state, its share, the entropy, and the change of composition from the bin before, whose jumps mark boundaries.
`track_lines(...)` writes a track in BED order, `tracks_files(...)` is the command line's --tracks FILE.mat.

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

from .maps import MAX_STATES, check_K, check_len_vec, check_state_vec, device, load_map, regions, stem

GRID_CAP = 1024                  # csrc/tracks.hip TRACKS_GRID_CAP: workgroups (of 256 lanes) of its kernel
TILE_H = 32                      # csrc/tracks.hip TRACKS_TILE_H: storage rows of the tile a workgroup counts at a time ...
TILE_W = 256                     # ... and TRACKS_TILE_W, its storage columns
MAX_WINDOWS = 8                  # distance windows of one --tracks run
HEADER = "#chrom\tstart\tstop\ttotal\tdominant\tshare\tentropy\tswitch"


def check_windows(windows):
    """-> int64 [Q, 2] of (d_min, d_max) in bins: d_min >= 0, d_max >= d_min or -1 for no upper limit; Q >= 1"""
    w = np.asarray(windows)
    if w.ndim != 2 or w.shape[1] != 2 or w.shape[0] < 1 or w.dtype.kind not in "iu":
        raise ValueError("windows must be a list of at least one (d_min, d_max) pair of integers")
    w = w.astype(np.int64)
    for lo, hi in w:
        if lo < 0 or (hi != -1 and hi < lo):
            raise ValueError("window (%d, %d): d_min must be >= 0 and d_max >= d_min, or -1 for no upper limit" % (lo, hi))
    return w


def parse_windows(text, resolution):
    """'lo-hi,lo-,...' in bp -> [(d_min, d_max), ...] in bins of `resolution` bp: d_min = ceil(lo / resolution), d_max =
    floor(hi / resolution), -1 for an open 'lo-'.  At most MAX_WINDOWS; a window that holds no whole bin distance is refused."""
    res = int(resolution)
    if res < 1:
        raise ValueError("resolution must be >= 1")
    parts = [p.strip() for p in str(text).split(",")]
    if not 1 <= len(parts) <= MAX_WINDOWS or not all(parts):
        raise ValueError("expected 1 to %d windows lo-hi or lo- separated by commas, got %r" % (MAX_WINDOWS, text))
    out = []
    for p in parts:
        lo, sep, hi = p.partition("-")
        if not sep or not lo.isdigit() or (hi and not hi.isdigit()):
            raise ValueError("a window is lo-hi or lo- with lo, hi in bp (non-negative integers), not %r" % p)
        d_min = -(-int(lo) // res)
        d_max = int(hi) // res if hi else -1
        if d_max != -1 and d_max < d_min:
            raise ValueError("the window %s holds no distance that is a multiple of the resolution %d" % (p, res))
        out.append((d_min, d_max))
    return out


def chromosomes(len_vec):
    """-> the chromosomes of len_vec, ascending"""
    return np.unique(np.asarray(len_vec)[:, 9]).astype(np.int64)


def covered_bins(len_vec, chrom):
    """-> bool [B]: the bins of the chromosome some region of len_vec covers with a row or a column (B: the largest
    start_bin + size over the chromosome's regions)"""
    rows = [r for r in np.asarray(len_vec) if int(r[9]) == int(chrom)]
    B = max([0] + [max(int(r[5]) + int(r[3]), int(r[6]) + int(r[4])) for r in rows])
    out = np.zeros(B, dtype=bool)
    for r in rows:
        out[int(r[5]):int(r[5]) + int(r[3])] = True
        out[int(r[6]):int(r[6]) + int(r[4])] = True        # (a diagonal region: the same bins once more)
    return out


def merge_tracks(rows, cols, len_vec, chrom):
    """The chromosome's track int64 [Q, B, K] from its regions' counts (rows[r] [Q, H, K], cols[r] [Q, W, K] or None for a
    diagonal region): rows at start_bin1 + i, an off-diagonal region's cols at start_bin2 + j -- the off-diagonal block
    stands for its mirror image too, so a bin's entry is its row of the chromosome's full matrix, restricted to the stored
    regions.  Host only."""
    Q, K = rows[0].shape[0], rows[0].shape[2]
    out = np.zeros((Q, covered_bins(len_vec, chrom).shape[0], K), dtype=np.int64)
    for r, row in enumerate(np.asarray(len_vec)):
        if int(row[9]) != int(chrom):
            continue
        H, W, s1, s2 = int(row[3]), int(row[4]), int(row[5]), int(row[6])
        out[:, s1:s1 + H] += rows[r]
        if not int(row[8]):
            out[:, s2:s2 + W] += cols[r]
    return out


def state_tracks(state_vec, len_vec, windows=((0, -1),), K=None):
    """Region by region and window by window -> dict:
      rows_<r> int64 [Q, H, K]           per row i of region r's full matrix: its cells inside window q in state k
      cols_<r> int64 [Q, W, K]           the same per column j (off-diagonal regions only: a diagonal region's equal its rows)
      chrom int64 [C]                    the chromosomes, ascending
      track_<chrom> int64 [Q, B, K]      the chromosome's merged track (merge_tracks); bins no region covers hold zeros
      windows int64 [Q, 2]               (d_min, d_max) in bins, d_max -1: no upper limit
    A cell (i, j) of a region has the distance |start_bin2 - start_bin1 + j - i|.  K: the largest state + 1 by default; a
    state >= K inside a window is an error, outside every window it is not looked at."""
    from . import _lib
    import torch
    s = check_state_vec(state_vec)
    L = check_len_vec(len_vec, s.shape[0])
    wins = check_windows(windows)
    K = check_K(s, K)
    lib, dev, stream = device()
    s_t = torch.from_numpy(s.astype(np.uint8)).to(dev)
    Q = wins.shape[0]
    out, rows, cols = {}, [], []
    for r, lo, hi, H, W, diag, dist0 in regions(L):
        rr = np.zeros((Q, H, K), dtype=np.int64)
        cc = None if diag else np.zeros((Q, W, K), dtype=np.int64)
        for q, (d_min, d_max) in enumerate(wins):
            _lib.check(lib.phmrf_state_tracks(ctypes.c_void_p(s_t[lo:hi].data_ptr()), H, W, diag, dist0, K,
                                              int(d_min), int(d_max), _lib.ptr_i64(rr[q]),
                                              None if diag else _lib.ptr_i64(cc[q]), stream))
        rows.append(rr)
        cols.append(cc)
        out["rows_%d" % r] = rr
        if not diag:
            out["cols_%d" % r] = cc
    out["chrom"] = chromosomes(L)
    for c in out["chrom"]:
        out["track_%d" % c] = merge_tracks(rows, cols, L, c)
    out["windows"] = wins
    return out


def track_summary(track):
    """track [B, K] (counts of one window) -> dict of [B] arrays, per bin:
      total float64       the bin's cells
      dominant int64      the state most of them hold, the lowest on ties; -1 for an empty bin
      share float64       that state's part of the total (NaN for an empty bin)
      entropy float64     of the bin's composition p, in bits (NaN for an empty bin)
      switch float64      0.5 sum_k |p[g][k] - p[g - 1][k]|, the total-variation distance to the bin before: 0 between equal
                          compositions, 1 between bins that share no state; NaN for the first bin and beside an empty bin
    Host only."""
    t = np.asarray(track)
    if t.ndim != 2 or t.shape[1] < 1 or t.dtype.kind not in "iu":
        raise ValueError("track_summary takes the integer counts [B, K] of one window (got %s %s)" % (t.dtype, t.shape))
    t = t.astype(np.float64)
    B = t.shape[0]
    total = t.sum(axis=1)
    full = total > 0
    p = np.zeros_like(t)
    p[full] = t[full] / total[full, None]
    dominant = np.where(full, np.argmax(t, axis=1), -1).astype(np.int64) if B else np.zeros(0, dtype=np.int64)
    share = np.where(full, p.max(axis=1), np.nan) if B else np.zeros(0)
    logs = np.zeros_like(p)
    logs[p > 0] = np.log2(p[p > 0])
    entropy = np.where(full, np.abs(-(p * logs).sum(axis=1)), np.nan)          # (abs: no -0.0)
    switch = np.full(B, np.nan)
    if B > 1:
        both = full[1:] & full[:-1]
        switch[1:] = np.where(both, 0.5 * np.abs(p[1:] - p[:-1]).sum(axis=1), np.nan)
    return dict(total=total, dominant=dominant, share=share, entropy=entropy, switch=switch)


def track_lines(tracks, len_vec, resolution, q):
    """-> the lines of tracks_*_w<q>.txt from state_tracks' dict, header first: one line per bin that a region covers, in BED
    order (chromosome, then start): chrom, start, stop, total, dominant + 1 (0: none), share, entropy, switch, the K counts.
    `switch` compares with the bin before on the genome, covered or not."""
    res = int(resolution)
    chrom = np.asarray(tracks["chrom"]).reshape(-1)
    K = tracks["track_%d" % chrom[0]].shape[2] if chrom.size else 0
    lines = [HEADER + "".join("\tstate%d" % (k + 1) for k in range(K)) + "\n"]
    for c in chrom:
        t = np.asarray(tracks["track_%d" % c])[q]
        sm = track_summary(t)
        for g in np.flatnonzero(covered_bins(len_vec, c)):
            lines.append("%d\t%d\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\t%s\n"
                         % (c, g * res, (g + 1) * res, sm["total"][g], sm["dominant"][g] + 1, sm["share"][g], sm["entropy"][g],
                            sm["switch"][g], "\t".join("%d" % x for x in t[g])))
    return lines


def tracks_files(path, output_path, resolution, field="state_vec", windows_bp="0-"):
    """The command line's --tracks: project the `field` of one estimate_ou_*.mat / segment_*.mat / smooth_*.mat.  Writes under
    output_path tracks_<stem>.npz (state_tracks' arrays, len_vec, resolution, tracks_field, windows_bp; no pickles) and per
    window q tracks_<stem>_w<q>.txt (track_lines).  -> the .npz"""
    res = int(resolution)
    if res < 1:
        raise ValueError("resolution must be >= 1")
    wins = parse_windows(windows_bp, res)
    s, L, _ = load_map(path, field)
    tracks = state_tracks(s, L, windows=wins)
    os.makedirs(output_path, exist_ok=True)
    name = stem(path)
    out = os.path.join(output_path, "tracks_%s.npz" % name)
    np.savez(out, len_vec=L, resolution=np.int64(res), tracks_field=np.array(field), windows_bp=np.array(str(windows_bp)),
             **tracks)
    for q in range(len(wins)):
        with open(os.path.join(output_path, "tracks_%s_w%d.txt" % (name, q)), "wb") as fh:
            fh.write("".join(track_lines(tracks, L, res, q)).encode())
    return out
