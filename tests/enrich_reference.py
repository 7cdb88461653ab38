"""The pair enrichment of a state map restated over the full index arrays of a region's stored nodes in NumPy (DESIGN.md
section 7; the definition the GPU's phmrf_pair_enrichment is held to) and the distance-matched expectation in float64.  Host
only, shares nothing with phylo_hmrf_amd.enrich."""
import numpy as np


def nodes(H, W, diag):
    """-> (i, j) of the stored nodes in node order"""
    if diag:
        return np.triu_indices(H)
    ii, jj = np.indices((H, W))
    return ii.reshape(-1), jj.reshape(-1)


def tables(labels, H, W, diag, dist0, K, C, row_class, col_class=None, row_seg=None, col_seg=None, d_min=0, d_max=-1,
           d_lo=0, D=None):
    """-> (obs int64 [2 C C, K], state_dist int64 [D, K], cat_dist int64 [D, 2 C C]) over the stored nodes inside the window;
    row 0 of the distance tables is the distance d_lo (D None: up to the largest distance inside the window).  A diagonal
    block takes its column values from the row arrays.  A state >= K or a class >= C inside the window is an error."""
    i, j = nodes(H, W, diag)
    if diag:
        col_class, col_seg = row_class, row_seg
    d = np.abs(int(dist0) + j - i)
    ok = (d >= d_min) & ((d <= d_max) if d_max != -1 else True)
    i, j, d, s = i[ok], j[ok], d[ok], np.asarray(labels).astype(np.int64)[ok]
    rc, cc = np.asarray(row_class).astype(np.int64)[i], np.asarray(col_class).astype(np.int64)[j]
    assert not np.any(s >= K) and not np.any(rc >= C) and not np.any(cc >= C)
    same = np.zeros(i.shape[0], dtype=np.int64)
    if row_seg is not None and col_seg is not None:
        rs, cs = np.asarray(row_seg).astype(np.int64)[i], np.asarray(col_seg).astype(np.int64)[j]
        same = ((rs >= 0) & (rs == cs)).astype(np.int64)
    p = (rc * C + cc) * 2 + same
    P = 2 * C * C
    if D is None:
        D = int(d.max()) - d_lo + 1 if d.size else 0
    assert not d.size or (d.min() >= d_lo and d.max() < d_lo + D)
    t = d - d_lo
    obs = np.bincount(p * K + s, minlength=P * K).reshape(P, K)
    state_dist = np.bincount(t * K + s, minlength=D * K).reshape(D, K)
    cat_dist = np.bincount(t * P + p, minlength=D * P).reshape(D, P)
    return obs.astype(np.int64), state_dist.astype(np.int64), cat_dist.astype(np.int64)


def expected(state_dist, cat_dist):
    """-> float64 [P, K]: sum over the distances d that hold a node of cat_dist[d][p] state_dist[d][k] / N[d]"""
    S, Cat = np.asarray(state_dist, dtype=np.float64), np.asarray(cat_dist, dtype=np.float64)
    out = np.zeros((Cat.shape[1], S.shape[1]))
    for d in range(S.shape[0]):
        N = S[d].sum()
        if N > 0:
            out += np.outer(Cat[d], S[d] / N)
    return out


def _take(table, chrom, start, count, fill):
    out = np.full(count, fill, dtype=np.int64)
    if table is not None and chrom in table:
        part = np.asarray(table[chrom])[start:start + count]
        out[:len(part)] = part
    return out


def pair_enrichment(state_vec, len_vec, bin_class, bin_seg, window, K, C):
    """-> dict(obs, obs_region, state_dist, cat_dist, d0, expected) summed over the regions on the distance axis from 0 that is
    then cut to the distances [d0, d0 + Dg) some region holds inside the window"""
    s, L = np.asarray(state_vec).reshape(-1), np.asarray(len_vec)
    far = int(max(abs(int(r[6]) - int(r[5])) + int(r[3]) + int(r[4]) for r in L))
    P = 2 * C * C
    S, Cat, regions = np.zeros((far, K), dtype=np.int64), np.zeros((far, P), dtype=np.int64), []
    seen = np.zeros(far, dtype=bool)
    for row in L:
        a, b, H, W, s1, s2, diag, chrom = (int(row[x]) for x in (1, 2, 3, 4, 5, 6, 8, 9))
        rs = cs = None
        if bin_seg is not None:
            rs, cs = _take(bin_seg, chrom, s1, H, -1), _take(bin_seg, chrom, s2, W, -1)
        obs, sd, cd = tables(s[a:b], H, W, diag, s2 - s1, K, C, _take(bin_class, chrom, s1, H, 0), _take(bin_class, chrom, s2, W, 0),
                             rs, cs, window[0], window[1], 0, far)
        regions.append(obs)
        S += sd
        Cat += cd
        i, j = nodes(H, W, diag)
        d = np.abs(s2 - s1 + j - i)
        seen[d[(d >= window[0]) & ((d <= window[1]) if window[1] != -1 else True)]] = True
    at = np.flatnonzero(seen)
    d0, d1 = (int(at[0]), int(at[-1]) + 1) if at.size else (int(window[0]), int(window[0]))
    return dict(obs=np.sum(regions, axis=0), obs_region=np.stack(regions), state_dist=S[d0:d1], cat_dist=Cat[d0:d1], d0=d0,
                expected=expected(S[d0:d1], Cat[d0:d1]))
