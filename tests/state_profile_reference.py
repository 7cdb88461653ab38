"""NumPy restatement of phmrf_state_hist, phmrf_state_moments and profile.state_profile (include/phmrf.h, DESIGN.md
section 7), written from the definitions alone: sorting instead of selecting, enumeration of the cells instead of the
closed form of a node's coordinates, exact sums (math.fsum) instead of any particular order of summation."""
import math

import numpy as np

BANDS = 32
SENTINEL = 0xFFFFFFFF


def order_key(x32):
    """orderable uint32 key of float32 values: ascending keys are ascending floats, -0 below +0"""
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def key_sort(v32):
    """float32 values in the order of their keys (np.sort's order, with -0 before +0)"""
    v32 = np.asarray(v32, dtype=np.float32)
    return v32[np.argsort(order_key(v32), kind="stable")]


def state_hist(x32, labels, K, shift, prefix=None):
    """-> uint64 [K, S, J, 256]; x32 float32 [n, S] and labels [n] are the OWNED nodes"""
    x32 = np.asarray(x32, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    n, S = x32.shape
    if shift == 24:
        prefix = np.zeros((K, S, 1), dtype=np.uint32)
    prefix = np.asarray(prefix, dtype=np.uint32)
    J = prefix.shape[2]
    keys = order_key(x32).astype(np.int64)
    hist = np.zeros((K, S, J, 256), dtype=np.uint64)
    ok = labels < K
    lab = np.where(ok, labels, 0)
    for s in range(S):
        digit = (keys[:, s] >> shift) & 255
        for j in range(J):
            m = ok.copy()
            if shift != 24:
                m &= (keys[:, s] >> (shift + 8)) == prefix[lab, s, j].astype(np.int64)
            hist[:, s, j, :] = np.bincount(lab[m] * 256 + digit[m], minlength=K * 256).reshape(K, 256)
    return hist


def cells(H, W, diagonal):
    """(i, j) of every node of a grid block in node order, by enumeration"""
    out = [(i, j) for i in range(H) for j in range(i if diagonal else 0, W)]
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def band_of(d):
    return 0 if d == 0 else int(d).bit_length()


def state_moments(x32, labels, K, geometry=None, dist0=0):
    """-> (count int64 [K], sum, sumsq float64 [K, S] correctly rounded, abs_sum, abs_sumsq = the sums of |term|, bands int64
    [K, 32] or None without a geometry (H, W, diagonal))"""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    S = x.shape[1]
    count = np.bincount(labels[labels < K], minlength=K).astype(np.int64)
    total, sq, a1 = np.zeros((K, S)), np.zeros((K, S)), np.zeros((K, S))
    for k in range(K):
        xk = x[labels == k]
        for s in range(S):
            total[k, s] = math.fsum(xk[:, s])
            sq[k, s] = math.fsum(xk[:, s] * xk[:, s])
            a1[k, s] = math.fsum(np.abs(xk[:, s]))
    bands = None
    if geometry is not None:
        ij = cells(*geometry)
        assert ij.shape[0] == labels.shape[0]
        bands = np.zeros((K, BANDS), dtype=np.int64)
        for (i, j), k in zip(ij.tolist(), labels.tolist()):
            if k < K:
                bands[k, band_of(abs(dist0 + j - i))] += 1
    return count, total, sq, a1, sq.copy(), bands


def order_statistics(x32, labels, K, ranks):
    """float32 [K, S, T]: the value at rank ranks[k, s, t] of the key-sorted values of (k, s); NaN where the rank is -1"""
    x32 = np.asarray(x32, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    ranks = np.asarray(ranks, dtype=np.int64)
    out = np.full(ranks.shape, np.nan, dtype=np.float32)
    for k in range(K):
        for s in range(x32.shape[1]):
            v = key_sort(x32[labels == k, s])
            for t in range(ranks.shape[2]):
                if ranks[k, s, t] >= 0:
                    out[k, s, t] = v[ranks[k, s, t]]
    return out


def make_run_pass(units, K):
    """run_pass of profile.select over `units` = [(x32, labels)], with a log of the prefix tables it was handed"""
    log = []

    def run_pass(shift, prefix):
        log.append((shift, np.array(prefix, copy=True)))
        total = None
        for x32, labels in units:
            h = state_hist(x32, labels, K, shift, prefix)
            total = h if total is None else total + h
        return total

    return run_pass, log


def state_profile(x32, labels, len_vec, K, quantiles):
    """the integer, order-statistic and moment fields of profile.state_profile from the gathered labels and float32
    observations of all samples"""
    x32 = np.asarray(x32, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    q = np.asarray(quantiles, dtype=np.float64)
    S = x32.shape[1]
    count, total, sq, a1, a2, _ = state_moments(x32, labels, K)
    count_region = np.zeros((len(len_vec), K), dtype=np.int64)
    bands = np.zeros((K, BANDS), dtype=np.int64)
    for r, lv in enumerate(len_vec):
        lab = labels[lv[1]:lv[2]]
        count_region[r] = np.bincount(lab, minlength=K)
        for (i, j), k in zip(cells(lv[3], lv[4], bool(lv[8])).tolist(), lab.tolist()):
            bands[k, band_of(abs(lv[6] - lv[5] + j - i))] += 1
    q_lo = np.full((K, S, q.size), np.nan, dtype=np.float32)
    q_hi = q_lo.copy()
    qv = np.full((K, S, q.size), np.nan)
    for k in range(K):
        if count[k] == 0:
            continue
        for s in range(S):
            v = key_sort(x32[labels == k, s])
            for t, qq in enumerate(q):
                h = (count[k] - 1) * float(qq)
                q_lo[k, s, t], q_hi[k, s, t] = v[int(math.floor(h))], v[int(math.ceil(h))]
            qv[k, s] = np.quantile(v.astype(np.float64), q)
    return dict(count=count, count_region=count_region, bands=bands, sum=total, sumsq=sq, abs_sum=a1, abs_sumsq=a2, q_lo=q_lo,
                q_hi=q_hi, q=qv)


FORMS = ("normal", "eighths", "constant", "signs", "topbyte")


def make_values(form, rng, n, S):
    """float64 [n, S] test observations: normal draws; multiples of 1/8 with heavy ties; a constant first column; mixed signs
    with +-0 and denormals; values of one binade and sign (every key shares its top byte)"""
    if form == "normal":
        return rng.normal(0.3, 1.0, (n, S))
    if form == "eighths":
        return rng.integers(-16, 17, (n, S)) / 8.0
    if form == "constant":
        x = rng.normal(0.3, 1.0, (n, S))
        x[:, 0] = 1.25
        return x
    if form == "signs":
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-42, -7e-41, 1e-39, -1e-39, 1.5, -1.5, 2.5e-38, -2.5e-38, 7.0, -0.125])
        return pool[rng.integers(0, pool.size, (n, S))]
    if form == "topbyte":
        return 1.0 + 0.96 * rng.random((n, S))
    raise ValueError(form)


def make_labels(kind, rng, n, K):
    """"runs": piecewise constant in long runs; "nodes": drawn per node (runs of length 1)"""
    if kind == "nodes":
        return rng.integers(0, K, n)
    out = np.empty(n, dtype=np.int64)
    pos = 0
    while pos < n:
        step = int(rng.integers(40, 400))
        out[pos:pos + step] = rng.integers(0, K)
        pos += step
    return out
