"""The k-means step of the initialisation (csrc/init.hip: kmeans_step_kernel<S, OUTER>) without a GPU: a float64 model,
inputs on which the kernel's float32 arithmetic is exact, the error bounds of real-valued inputs, a float32 emulation of
the kernel's accumulation scheme, and the case list that tests/test_kmeans_reference.py (CPU) and
tests/test_gpu_kmeans.py (device) share.

What the kernel computes, per node i (one thread) and in this order:
  t_s = x_s - c_ks                      one f32 subtraction
  d_k = fma(t_s, t_s, d_k)              s = 0 .. S-1, starting from 0: one rounding per s
  label = first k with the smallest d_k (strict <, ascending k)
and, for the nodes in [own0, own1) only, into the workgroup's f32 LDS slots by atomic adds in arbitrary order
  sums[label, s] += x_s,  counts[label] += 1,  inertia += d_label,  outer[label, s, t] += x_s * x_t (one f32 product)
After each tile of 256 nodes the slots are added to the f64 accumulators (f64 atomics, arbitrary order) and zeroed.

BOUNDS for inputs that are float32 numbers, u = 2^-24 (f32 unit roundoff), u64 = 2^-53:

distance   t^ = t (1 + e), |e| <= u.  Term s of d^ carries (1 + e_s)^2 from the square and one factor (1 + e') per fma from
           s on: at most S + 2 factors, all terms are >= 0, so d^ = d (1 + th), |th| <= (1 + u)^(S+2) - 1 < (S + 3) u.
label      the device takes b where the model takes r != b only if d^_b <= d^_r, that is d_b (1 - th) <= d_r (1 + th):
           d_b - d_r <= th (d_b + d_r) <= 2 (S + 3) u max(d_b, d_r).                                   [label_slack]
           Such a node has its two smallest distances within that slack (d_(2) <= d_b): the nodes near_ties() counts.
counts     integers <= 256 in f32, integers in f64: exact.  counts == bincount(device labels over own).
sums       over the DEVICE's labels.  A tile's slot is an f32 sum of m <= 256 terms in some order: |error| <= (m - 1) u
outer      sum|term| (Jeannerod & Rump 2013, "Improved error bounds for inner products in floating-point arithmetic":
           no higher-order term, any order).  The terms of outer are the f32 products x_s * x_t the kernel forms (one
           rounding each, the same in every IEEE implementation): the model forms the same f32 products and sums them
           in f64, so the comparison is of the accumulation.  The f64 atomics add T = ceil(n / 256) partial sums, each
           within (1 + 255 u) of its terms' absolute sum: <= (T - 1) u64 (1 + 255 u) sum|term|; the model's own f64
           sum over the n_k terms of a cluster adds <= n_k u64 sum|term|.  Per entry:
              255 u sum|term|  +  (T + n) u64 (1 + 255 u) sum|term|                                     [sum_bound]
inertia    against I = sum_i d[i, label_i] (f64 distances at the device's labels): each added value is d (1 + th), the tile
           sum adds 255 u, the f64 part (T u64 < 2^-40 for every n below 2^21) and the products of the three are inside
           the step from (S + 2) to (S + 3):  |inertia - I| <= (S + 3 + 255) u I.                      [inertia_bound]

DYADIC inputs (dyadic_case): X and the centres are multiples of 1/8 in [0, 4).  Then t is a multiple of 1/8 with |t| < 4,
t^2 a multiple of 1/64 below 16, every d_k a multiple of 1/64 below 256 (S <= 16): 2^14 steps.  A tile's sums are multiples
of 1/8 below 256 * 4 = 2^10, its products multiples of 1/64 below 256 * 16 = 2^12, its inertia a multiple of 1/64 below
256 * 256 = 2^16: 2^22 steps.  All of it fits f32's 24 bits, and the f64 totals are below 2^53 steps for every n below
2^31: every operation is exact in any order, and the device must return the model's numbers bit for bit.
"""
import functools

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
TILE = 256                    # nodes per workgroup trip (launch_kmeans_step)
GRID_CAP = 2048               # workgroups at most: above GRID_CAP * TILE nodes a workgroup takes a second trip
KSET = (1, 2, 3, 7, 20, 63, 64)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _chunks(n, K, S):
    rows = max(1, (1 << 21) // (K * S))        # (the [rows, K, S] broadcast stays near 16 MB)
    for a in range(0, n, rows):
        yield a, min(n, a + rows)


def two_smallest(X, C):
    """-> (labels[n] = first index of the smallest float64 distance, d1[n] that distance, d2[n] the second smallest or inf)"""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    n, K = X.shape[0], C.shape[0]
    lab, d1, d2 = np.empty(n, dtype=np.int64), np.empty(n), np.full(n, np.inf)
    for a, b in _chunks(n, K, X.shape[1]):
        d = ((X[a:b, None, :] - C[None, :, :]) ** 2).sum(axis=2)
        lab[a:b] = np.argmin(d, axis=1)
        if K > 1:
            p = np.partition(d, 1, axis=1)
            d1[a:b], d2[a:b] = p[:, 0], p[:, 1]
        else:
            d1[a:b] = d[:, 0]
    return lab, d1, d2


def distance_at(X, C, lab):
    """float64 |x_i - c_lab[i]|^2"""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    return ((X - C[lab]) ** 2).sum(axis=1)


def moments(X, lab, K, own=None):
    """float64 sums over the nodes [own) with the given labels -> (counts[K], sums[K,S], outer[K,S,S], and the sums of
    the absolute terms abs_sums[K,S], abs_outer[K,S,S]).  The terms of outer are the float32 products x_s * x_t."""
    X = np.asarray(X, dtype=np.float64)
    n, S = X.shape
    lo, hi = (0, n) if own is None else own
    x, l = X[lo:hi], np.asarray(lab)[lo:hi]
    counts = np.bincount(l, minlength=K).astype(np.float64)
    sums, abs_sums = np.zeros((K, S)), np.zeros((K, S))
    outer, abs_outer = np.zeros((K, S, S)), np.zeros((K, S, S))
    x32 = x.astype(np.float32)
    for s in range(S):
        sums[:, s] = np.bincount(l, weights=x[:, s], minlength=K)
        abs_sums[:, s] = np.bincount(l, weights=np.abs(x[:, s]), minlength=K)
        for t in range(S):
            p = (x32[:, s] * x32[:, t]).astype(np.float64)
            outer[:, s, t] = np.bincount(l, weights=p, minlength=K)
            abs_outer[:, s, t] = np.bincount(l, weights=np.abs(p), minlength=K)
    return counts, sums, outer, abs_sums, abs_outer


def step(X, C, own=None):
    """The model: -> (labels[n], counts[K], sums[K,S], outer[K,S,S], inertia).  Every node is labelled (float64 distances,
    lowest index on ties); the statistics run over the nodes [own[0], own[1]) only (default: all)."""
    X = np.asarray(X, dtype=np.float64)
    lab, d1, _ = two_smallest(X, C)
    lo, hi = (0, X.shape[0]) if own is None else own
    counts, sums, outer, _, _ = moments(X, lab, len(C), own)
    return lab, counts, sums, outer, float(d1[lo:hi].sum())


# ---- bounds ------------------------------------------------------------------------------------------------------------
def label_slack(S, da, db):
    return 2.0 * (S + 3) * U * np.maximum(da, db)


def near_ties(X, C):
    """the nodes whose two smallest float64 distances lie within label_slack of each other: where a float32 label may differ"""
    _, d1, d2 = two_smallest(X, C)
    near = np.isfinite(d2)                     # (K = 1: there is no second centre)
    near[near] = (d2 - d1)[near] <= label_slack(np.shape(X)[1], d1, d2)[near]
    return np.flatnonzero(near)


def tie_cap(n):
    return max(2, n // 1000)


def sum_bound(abs_terms, n):
    tiles = (n + TILE - 1) // TILE
    return (255.0 * U + (tiles + n) * U64 * (1.0 + 255.0 * U)) * abs_terms


def inertia_bound(S, inertia):
    return (S + 3 + 255) * U * inertia


def check_exact(X, C, got, own=None, with_outer=True):
    """dyadic inputs: `got` = (labels or None, counts, sums, outer or None, inertia) equals the model bit for bit"""
    lab, counts, sums, outer, inertia = step(X, C, own)
    g_lab, g_counts, g_sums, g_outer, g_inertia = got
    if g_lab is not None:
        bad = np.flatnonzero(np.asarray(g_lab) != lab)
        assert bad.size == 0, "labels differ at %d nodes, first %s" % (bad.size, bad[:5])
    assert np.array_equal(g_counts, counts), ("counts", g_counts, counts)
    assert np.array_equal(g_sums, sums), ("sums", np.abs(g_sums - sums).max())
    assert g_inertia == inertia, ("inertia", g_inertia, inertia)
    if with_outer:
        assert np.array_equal(g_outer, outer), ("outer", np.abs(g_outer - outer).max())


def check_real(X, C, got, own=None, with_outer=True):
    """float32-valued inputs: `got` = (labels, counts, sums, outer or None, inertia) within the bounds of the module's
    docstring.  -> the measured figures, each as a fraction of its bound (for printing)."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    n, S = X.shape
    K = C.shape[0]
    lo, hi = (0, n) if own is None else own
    g_lab, g_counts, g_sums, g_outer, g_inertia = got
    g_lab = np.asarray(g_lab, dtype=np.int64)
    assert g_lab.shape == (n,) and g_lab.min() >= 0 and g_lab.max() < K
    lab, d1, _ = two_smallest(X, C)
    diff = np.flatnonzero(g_lab != lab)
    d_dev = distance_at(X[diff], C, g_lab[diff])
    assert np.all(d_dev - d1[diff] <= label_slack(S, d_dev, d1[diff])), "a label differs from the model's without a tie"
    assert diff.size <= tie_cap(n), (diff.size, tie_cap(n))
    counts, sums, outer, abs_sums, abs_outer = moments(X, g_lab, K, own)
    assert np.array_equal(g_counts, counts), ("counts", g_counts, counts)
    figures = {"labels": int(diff.size)}
    err, bound = np.abs(g_sums - sums), sum_bound(abs_sums, n)
    figures["sums"] = float(np.max(err / np.where(bound > 0, bound, 1.0)))
    assert np.all(err <= bound), ("sums", figures["sums"])
    if with_outer:
        err, bound = np.abs(g_outer - outer), sum_bound(abs_outer, n)
        figures["outer"] = float(np.max(err / np.where(bound > 0, bound, 1.0)))
        assert np.all(err <= bound), ("outer", figures["outer"])
    ref_inertia = float(distance_at(X[lo:hi], C, g_lab[lo:hi]).sum())
    figures["inertia"] = abs(g_inertia - ref_inertia) / max(inertia_bound(S, ref_inertia), 1e-300)
    assert abs(g_inertia - ref_inertia) <= inertia_bound(S, ref_inertia), ("inertia", g_inertia, ref_inertia)
    return figures


# ---- the kernel's scheme in NumPy float32 ------------------------------------------------------------------------------
def emulate(X, C, own=None, rng=None):
    """kmeans_step_kernel<S, true>'s scheme in float32: distances by a near-fma (below), strict < in ascending k, per tile
    of 256 nodes the f32 slots filled in a shuffled node order, then added to float64 totals.  NumPy has no fma: t * t is
    formed exactly in float64, but d + t * t is then rounded to float64 and again to float32, which in rare cases differs
    from fmaf's single rounding by one ulp.  The dyadic cases are exact either way, and the bounds cover both.
    -> (labels, counts, sums, outer, inertia)"""
    rng = np.random.default_rng(0) if rng is None else rng
    X32, C32 = np.asarray(X, dtype=np.float32), np.asarray(C, dtype=np.float32)
    n, S = X32.shape
    K = C32.shape[0]
    lo, hi = (0, n) if own is None else own
    best = np.full(n, np.float32(3.0e38))
    lab = np.zeros(n, dtype=np.int64)
    for k in range(K):
        d = np.zeros(n, dtype=np.float32)
        for s in range(S):
            t = X32[:, s] - C32[k, s]                                             # f32
            d = (d.astype(np.float64) + t.astype(np.float64) ** 2).astype(np.float32)   # t * t exact, the sum rounded twice
        closer = d < best
        best[closer], lab[closer] = d[closer], k
    T = (n + TILE - 1) // TILE
    pad = T * TILE - n
    idx = np.concatenate([np.arange(n), np.full(pad, -1)]).reshape(T, TILE)
    idx = rng.permuted(idx, axis=1)                                               # every tile in an order of its own
    rows = np.arange(T)
    p_sums = np.zeros((T, K, S), dtype=np.float32)
    p_counts = np.zeros((T, K), dtype=np.float32)
    p_inertia = np.zeros(T, dtype=np.float32)
    p_outer = np.zeros((T, K, S, S), dtype=np.float32)
    for j in range(TILE):
        i = idx[:, j]
        live = (i >= lo) & (i < hi)
        r, ii = rows[live], i[live]
        l = lab[ii]
        x = X32[ii]
        p_sums[r, l] += x
        p_counts[r, l] += np.float32(1)
        p_inertia[r] += best[ii]
        p_outer[r, l] += x[:, :, None] * x[:, None, :]
    f = lambda a: a.astype(np.float64).sum(axis=0)
    return lab, f(p_counts), f(p_sums), f(p_outer), float(f(p_inertia))


# ---- inputs ------------------------------------------------------------------------------------------------------------
def dyadic_case(rng, n, S, K):
    """-> (X[n,S], C[K,S]) in multiples of 1/8 in [0, 4), with exact ties planted:
      K >= 2  centre 1 = centre 0 + 2/8 along the first coordinate, and max(1, n // 16) nodes placed at centre 0 + 1/8,
              exactly midway (distance^2 1/64 to both, the smallest non-zero one there is; a random centre that fell on
              that very point is moved onto centre 0, so the tie is at the minimum)
      K >= 3  centre K - 1 duplicates centre 0;   K >= 5  centre K - 2 duplicates centre 2
    (a duplicate of a lower centre never wins: its cluster stays empty)"""
    X = rng.integers(0, 32, (n, S)) / 8.0
    C = rng.integers(0, 32, (K, S)) / 8.0
    if K >= 2:
        C[0, 0] = rng.integers(0, 30) / 8.0
        C[1] = C[0]
        C[1, 0] += 2.0 / 8.0
        x_mid = C[0].copy()
        x_mid[0] += 1.0 / 8.0
        C[2:][np.all(C[2:] == x_mid, axis=1)] = C[0]          # no other centre sits on the midway point itself
        mid = rng.choice(n, size=min(n, max(1, n // 16)), replace=False)
        X[mid] = C[0]
        X[mid, 0] += 1.0 / 8.0
    if K >= 3:
        C[K - 1] = C[0]
    if K >= 5:
        C[K - 2] = C[2]
    return X, C


def midway_nodes(X, C):
    """the nodes of a dyadic case that sit at centre 0 + 1/8 along the first coordinate (K >= 2: exactly midway to centre 1)"""
    x = np.asarray(C, dtype=np.float64)[0].copy()
    x[0] += 1.0 / 8.0
    return np.flatnonzero(np.all(np.asarray(X) == x, axis=1))


def real_case(rng, n, S, K):
    """float32-valued observations and centres, uniform in [0, 4)^S"""
    return f32(rng.uniform(0.0, 4.0, (n, S))), f32(rng.uniform(0.0, 4.0, (K, S)))


class Case(object):
    def __init__(self, entry, S, K, n, kind):
        self.entry, self.S, self.K, self.n, self.kind = entry, S, K, n, kind
        rng = np.random.default_rng([S, K, n, int(kind == "dyadic"), int(entry == "moments")])
        self.X, self.C = (dyadic_case if kind == "dyadic" else real_case)(rng, n, S, K)
        self.with_outer = entry == "moments"

    def check(self, got, own=None):
        if self.kind == "dyadic":
            return check_exact(self.X, self.C, got, own, self.with_outer)
        return check_real(self.X, self.C, got, own, self.with_outer)


@functools.lru_cache(maxsize=2)
def case(entry, S, K, n, kind):
    return Case(entry, S, K, n, kind)


def case_id(c):
    return "%s-S%d-K%d-n%d-%s" % c


def _real_n(K):
    """n / K of a few hundred to a few thousand: one node more or less in a cluster is far outside sum_bound"""
    return min(max(300 * K, 3000), 19200) + 1


# every compiled form: S = 1 .. 16 without second moments (kmeans_step), S = 1 .. 8 with (kmeans_moments); K runs through
# KSET in both, and K = 64 at S = 8 with moments is the largest LDS and accumulator footprint the API admits
FORM_CASES = []
for _S in range(1, 17):
    _K = KSET[(_S - 1) % 7]
    FORM_CASES += [("step", _S, _K, 700 + 37 * _S, "dyadic"), ("step", _S, _K, _real_n(_K), "real")]
for _S in range(1, 9):
    _K = KSET[(_S + 5) % 7]
    FORM_CASES += [("moments", _S, _K, 700 + 37 * _S, "dyadic"), ("moments", _S, _K, _real_n(_K), "real")]
# the edges of the 256-node tile, on the scalar (S = 3) and the float4 (S = 4) load path
EDGE_CASES = [(e, S, 3, n, "dyadic") for n in (1, 255, 256, 257, 511, 513) for S in (3, 4) for e in ("step", "moments")]
# above GRID_CAP * TILE nodes workgroups 0 .. 1 take a second trip on zeroed slots; workgroup 1's second tile is partial
TRIP_N = GRID_CAP * TILE + 300
TRIP_CASES = [(e, S, 5, TRIP_N, "dyadic") for S in (3, 4) for e in ("step", "moments")]
CASES = FORM_CASES + EDGE_CASES + TRIP_CASES
