"""The genome tracks of a state map restated on the region's full matrix in NumPy (the definition the
GPU's phmrf_state_tracks is held to), the chromosome merge and the per-bin summary.  Host only, shares nothing with
phylo_hmrf_amd.tracks."""
import math

import numpy as np


def full(values, H, W, diag):
    """node order -> the H x W matrix: a diagonal block's upper triangle mirrored"""
    values = np.asarray(values)
    if not diag:
        return values.reshape(H, W).copy()
    M = np.zeros((H, H), dtype=values.dtype)
    iu = np.triu_indices(H)
    M[iu] = values
    M.T[iu] = values
    return M


def inside(H, W, dist0, d_min, d_max):
    """-> bool [H, W]: the cells with d_min <= |dist0 + j - i| and (d_max == -1 or |dist0 + j - i| <= d_max)"""
    ii, jj = np.indices((H, W))
    d = np.abs(int(dist0) + jj - ii)
    return (d >= d_min) & ((d <= d_max) if d_max != -1 else True)


def tracks(labels, H, W, diag, dist0, K, d_min, d_max):
    """-> (rows int64 [H, K], cols int64 [W, K]): per row and per column of the full matrix, the cells inside the window per
    state.  A state >= K inside the window is an error; outside it is not looked at."""
    M = full(np.asarray(labels).astype(np.int64), H, W, diag)
    ok = inside(H, W, dist0, d_min, d_max)
    assert not np.any(M[ok] >= K)
    rows = np.stack([np.bincount(M[i][ok[i]], minlength=K)[:K] for i in range(H)]).astype(np.int64)
    cols = np.stack([np.bincount(M[:, j][ok[:, j]], minlength=K)[:K] for j in range(W)]).astype(np.int64)
    return rows, cols


def state_tracks(state_vec, len_vec, windows, K):
    """-> dict(rows_<r> [Q, H, K], cols_<r> [Q, W, K] for the off-diagonal regions, track_<chrom> [Q, B, K], chrom)"""
    s, L = np.asarray(state_vec).reshape(-1), np.asarray(len_vec)
    out, per_region = {}, []
    for r, row in enumerate(L):
        a, b, H, W, s1, s2, diag = (int(row[x]) for x in (1, 2, 3, 4, 5, 6, 8))
        got = [tracks(s[a:b], H, W, diag, s2 - s1, K, lo, hi) for lo, hi in windows]
        rows, cols = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
        out["rows_%d" % r] = rows
        if not diag:
            out["cols_%d" % r] = cols
        per_region.append((rows, cols))
    out["chrom"] = np.unique(L[:, 9])
    for c in out["chrom"]:
        mine = [r for r in range(L.shape[0]) if L[r, 9] == c]
        B = max(max(int(L[r, 5] + L[r, 3]), int(L[r, 6] + L[r, 4])) for r in mine)
        t = np.zeros((len(windows), B, K), dtype=np.int64)
        for r in mine:
            rows, cols = per_region[r]
            for i in range(int(L[r, 3])):
                t[:, int(L[r, 5]) + i] += rows[:, i]
            if not int(L[r, 8]):
                for j in range(int(L[r, 4])):
                    t[:, int(L[r, 6]) + j] += cols[:, j]
        out["track_%d" % c] = t
    return out


def summary(track):
    """track [B, K] -> dict of lists per bin, in plain Python: total, dominant (-1: empty), share, entropy (bits), switch"""
    t = [[int(x) for x in row] for row in np.asarray(track)]
    out = dict(total=[], dominant=[], share=[], entropy=[], switch=[])
    before = None
    for row in t:
        total = sum(row)
        p = [x / total for x in row] if total else None
        out["total"].append(float(total))
        out["dominant"].append(row.index(max(row)) if total else -1)
        out["share"].append(max(p) if total else math.nan)
        out["entropy"].append(-sum(x * math.log2(x) for x in p if x > 0) if total else math.nan)
        out["switch"].append(0.5 * sum(abs(x - y) for x, y in zip(p, before)) if (p and before) else math.nan)
        before = p
    return out
