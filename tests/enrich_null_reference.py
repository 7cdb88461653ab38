"""The enrichment's permutation null restated in NumPy and Python integers (the definition the GPU's
phmrf_pair_enrichment_null is held to): per shift the padded chromosome arrays are rolled, the region's rows and columns are
sliced out of them, tests/enrich_reference.tables counts, and the fixed-point expectation is formed with Python integers.  Host
only, imports nothing from phylo_hmrf_amd.enrich."""
import numpy as np

from tests import enrich_reference as R

ONE = 1 << 24


def weights(state_dist):
    """-> Python-integer rows w[d][k] = (S[d][k] ONE) // N[d], zero where N[d] = 0, as an object array [D, K]"""
    S = np.asarray(state_dist)
    out = np.zeros(S.shape, dtype=object)
    for d in range(S.shape[0]):
        N = sum(int(x) for x in S[d])
        for k in range(S.shape[1]):
            out[d, k] = (int(S[d, k]) * ONE) // N if N else 0
    return out


def expq(cat_dist, w):
    """-> int64 [P, K]: sum_d Cat[d][p] w[d][k] in Python integers"""
    Cat, w = np.asarray(cat_dist), np.asarray(w).astype(object)
    out = np.zeros((Cat.shape[1], w.shape[1]), dtype=object)
    held = np.flatnonzero(Cat.any(axis=0))                    # (object arithmetic is slow: the categories that occur)
    if Cat.shape[0] and held.size:
        out[held] = Cat[:, held].astype(object).T.dot(w)
    assert all(0 <= int(x) < (1 << 63) for x in out.reshape(-1))
    return out.astype(np.int64)


def shifted(chrom_class, chrom_seg, B, s):
    """the chromosome's arrays padded (class 0, segment -1) or cut to B bins and moved by s: out[g] = in[(g + s) mod B]"""
    cls, seg = np.zeros(B, dtype=np.int64), np.full(B, -1, dtype=np.int64)
    a = np.asarray(chrom_class).reshape(-1)[:B]
    cls[:a.shape[0]] = a
    if chrom_seg is not None:
        b = np.asarray(chrom_seg).reshape(-1)[:B]
        seg[:b.shape[0]] = b
    return np.roll(cls, -int(s)), (np.roll(seg, -int(s)) if chrom_seg is not None else None)


def tables(labels, H, W, diag, row0, col0, K, C, chrom_class, chrom_seg, B, shifts, w, d_min=0, d_max=-1, d_lo=0, D=None):
    """-> (obs int64 [T, 2 C C, K], expq int64 [T, 2 C C, K]) of one region against the shifts; w: integer [D, K], row 0 the
    distance d_lo"""
    obs, exp = [], []
    for s in shifts:
        cls, seg = shifted(chrom_class, chrom_seg, B, s)
        o, _, cd = R.tables(labels, H, W, diag, col0 - row0, K, C, cls[row0:row0 + H], cls[col0:col0 + W],
                            None if seg is None else seg[row0:row0 + H], None if seg is None else seg[col0:col0 + W], d_min, d_max,
                            d_lo, D if D is not None else np.asarray(w).shape[0])
        obs.append(o)
        exp.append(expq(cd, w))
    return np.stack(obs), np.stack(exp)


def genome(state_vec, len_vec, bin_class, bin_seg, window, K, C, shifts):
    """-> dict(obs, expq [P, K] of the unshifted annotation, null_obs, null_expq [T, P, K], weights): summed over the
    regions; shifts {chrom: [T]}; chromosome c has B_c = the largest start_bin + size of its regions"""
    s, L = np.asarray(state_vec).reshape(-1), np.asarray(len_vec)
    base = R.pair_enrichment(s, L, bin_class, bin_seg, window, K, C)
    w = weights(base["state_dist"])
    d0 = int(base["d0"])
    T = len(next(iter(shifts.values())))
    P = 2 * C * C
    null_obs, null_expq = np.zeros((T, P, K), dtype=np.int64), np.zeros((T, P, K), dtype=np.int64)
    for row in L:
        a, b, H, W, s1, s2, diag, chrom = (int(row[x]) for x in (1, 2, 3, 4, 5, 6, 8, 9))
        B = max(max(int(r[5]) + int(r[3]), int(r[6]) + int(r[4])) for r in L if int(r[9]) == chrom)
        i, j = R.nodes(H, W, diag)
        d = np.abs(s2 - s1 + j - i)
        d = d[(d >= window[0]) & ((d <= window[1]) if window[1] != -1 else True)]
        if not d.size:
            continue
        d_lo, D = int(d.min()), int(d.max()) - int(d.min()) + 1
        o, e = tables(s[a:b], H, W, diag, s1, s2, K, C, (bin_class or {}).get(chrom, []),
                      None if bin_seg is None else bin_seg.get(chrom, []), B, shifts[chrom], w[d_lo - d0:d_lo - d0 + D], window[0],
                      window[1], d_lo, D)
        null_obs += o
        null_expq += e
    return dict(obs=base["obs"], expq=expq(base["cat_dist"], w), null_obs=null_obs, null_expq=null_expq,
                weights=w.astype(np.int64), state_dist=base["state_dist"], cat_dist=base["cat_dist"], expected=base["expected"])
