"""The cases of tests/test_gpu_posterior.py, without a GPU: the shapes the launcher's rule gives (tile rows, grid caps),
the graphs, labellings and inputs of each case with its float64 reference (tests/posterior_reference.py), and the
tolerances.  tests/test_posterior_reference.py checks on the CPU that the cases cover what they claim."""
import functools

import numpy as np

from oracle import ref_numpy as R
from tests import posterior_reference as P

FORMS = ("grid_diag", "grid_rect", "explicit8", "ragged4", "deg12", "isolated")
KEYS = ("post", "obs", "obs*obs.T")


def _block(n, S, K):
    from phylo_hmrf_amd import Block
    return Block(n, S, K)


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def tile_rows(K, S):
    """launch_posterior_s: 256 rows, halved while the tile ([TB][Kp + Mp] f32) and the K * M f64 accumulators exceed 64 KB - 256"""
    Kp = K + 1 if K % 2 == 0 else K
    M = 1 + S + S * (S + 1) // 2
    Mp = S + 2 if (S + 1) % 2 == 0 else S + 1
    TB = 256
    while TB > 64 and TB * (Kp + Mp) * 4 + K * M * 8 > 64 * 1024 - 256:
        TB >>= 1
    return TB, TB * (Kp + Mp) * 4 + K * M * 8


def default_wrap_nodes(K, S):
    """launch_posterior_s: workgroups are capped by the LDS class; above cap * (256 / TB) * TB nodes a workgroup takes a second tile"""
    _, lds = tile_rows(K, S)
    cap = 256 * 5 if lds <= 32 * 1024 else 256 * 4 if lds <= 40 * 1024 else 256 * 3 if lds <= 53 * 1024 else 256 * 8
    return cap * 256


# ---- graphs ----------------------------------------------------------------------------------------------------------
def _random_graph(rng, n, max_deg, attempts):
    """a random simple graph of degree <= max_deg on nodes 1 .. n - 1 (node 0 stays isolated), as test_gpu_segment's _ragged_graph"""
    deg = np.zeros(n, dtype=np.int64)
    seen, out = set(), []
    if n > 2:
        for _ in range(attempts):
            a, b = (int(v) for v in rng.integers(1, n, 2))
            if a == b or deg[a] >= max_deg or deg[b] >= max_deg or (min(a, b), max(a, b)) in seen:
                continue
            seen.add((min(a, b), max(a, b)))
            deg[a] += 1
            deg[b] += 1
            out.append((min(a, b), max(a, b)))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2), deg


def _rect(n):
    """n = H * W with 2 <= H <= W, H as large as it goes up to 16 (a stencil with more than four neighbours: D == 8), else None"""
    for H in range(16, 1, -1):
        if n % H == 0 and n // H >= H:
            return H, n // H
    return None


def _observations(rng, n, S):
    return _f32(np.minimum(np.abs(rng.standard_normal((n, S))) + 0.01, 3.99))


def _graph(rng, form, n, X):
    """-> (eid[E,2], w[E] f32-representable, geometry (H, W, diagonal) or None)"""
    geom = None
    if form in ("grid_diag", "grid_rect", "explicit8"):
        if form == "grid_diag":
            N = int(round((np.sqrt(8 * n + 1) - 1) / 2))
            assert N * (N + 1) // 2 == n and N >= 3, n
            H, W, diag = N, N, True
        else:
            H, W = _rect(n)
            diag = False
        e = R.grid_edges(X, H, W, diag, 8)
        w, eid = R.edge_weights_from_distance(e, 0.5)
        geom = (H, W, diag)
    elif form == "ragged4":
        eid, _ = _random_graph(rng, n, 4, 3 * n)
        w = rng.uniform(0.2, 1.0, len(eid))
    elif form == "deg12":
        eid, _ = _random_graph(rng, n, 12, 12 * n)
        w = rng.uniform(0.2, 1.0, len(eid))
    else:                                   # isolated: ragged rows of up to 6 neighbours, then every edge of ~ 15 % of the nodes cut
        eid, _ = _random_graph(rng, n, 6, 5 * n)
        cut = rng.random(n) < 0.15
        eid = eid[~(cut[eid[:, 0]] | cut[eid[:, 1]])] if len(eid) else eid
        w = rng.uniform(0.2, 1.0, len(eid))
    return eid, _f32(w), geom


def _labels(rng, mode, lp):
    n, K = lp.shape
    if mode == "random":
        return rng.integers(0, K, n)
    if mode == "argmax":
        return np.where(rng.random(n) < 0.8, np.argmax(lp, 1), rng.integers(0, K, n))
    if mode == "one":
        return np.full(n, K // 2, dtype=np.int64)
    lab = rng.integers(0, K, n)             # absent: state K - 1 labels no node (its statistics are not zero for that)
    lab[lab == K - 1] = 0
    return lab


# ---- the comparison ----------------------------------------------------------------------------------------------------
RTOL_COST = 1e-5


def _cost1_atol(labels, eid, w, K, beta, et):
    """The absolute term of cost [1] = sum_i t_i, t_i = -log(ppn_i + 1e-16): the f32 error of the nodes at which rtol * t_i
    is below the rounding of ppn itself, and nothing for the others -- a case without such nodes keeps the pure rtol.

    Where the label is the row maximum of a = beta * (h - Wtot), ppn = 1 / (1 + y) with y = sum_{k != l} e^(a_k - a_l) =
    e^t - 1, and the absolute error of the device's t = log(1 + y) is at most, in units of 2^-23:
      the label's own term   the shift is the same f32 expression as a_l, e_l = __expf(0) = 1: exact
      the K - 1 additions    2^-24 each, relative to a partial sum <= 1 + y; d log(1 + y) = dy / (1 + y)          K / 2
      the division, ppn + 1e-16f, logf: half an ulp of a number in (1/2, 1] each, and a spare one                   2
      the other e_k          x = a_k - max a: subtraction, product, shift -> |dx| <= 5 * 2^-24 beta Wtot; __expf adds
                             2^-23 (1 + |x|), |x| <= beta Wtot: relative <= (2 + 5 beta Wtot) on the sum y
                                                                                                y (2 + 5 beta Wtot_i)
    The first two lines do not shrink with t: a node with rtol * t_i < (2 + K / 2) * 2^-23 cannot meet rtol in f32, and those
    nodes get the whole bound.  K <= 64 keeps them at t < 0.41 < log 2, where the label is the row maximum.  Wtot_i is
    the node's own weight sum (1 for an isolated node: h = onehot, Wtot = 1)."""
    n = len(labels)
    ww = np.asarray(w, dtype=np.float64) if et == 3 else np.ones(len(eid))
    wtot = np.bincount(eid.ravel(), weights=np.concatenate([ww, ww]), minlength=n) if len(eid) else np.zeros(n)
    wtot = np.where(wtot > 0.0, wtot, 1.0)
    pp = R.pairwise_compare(labels, eid, w, R.potts_matrix(K, beta), et)
    t = -np.log(P.softmax_rows(-pp)[np.arange(n), labels] + R.SMALL_EPS)
    lattice = (2.0 + K / 2.0) * 2.0 ** -23
    near = t < min(lattice / RTOL_COST, np.log(2.0))
    return float(np.sum(lattice + np.expm1(np.maximum(t[near], 0.0)) * (2.0 + 5.0 * beta * wtot[near]) * 2.0 ** -23))


def _assert_costs(costs, ref, atol1):
    """rtol 1e-5 on all four; [1], and [3] which contains it, with the absolute term of _cost1_atol"""
    np.testing.assert_allclose(costs[0], ref[0], rtol=RTOL_COST)
    np.testing.assert_allclose(costs[1], ref[1], rtol=RTOL_COST, atol=atol1)
    np.testing.assert_allclose(costs[2], ref[2], rtol=RTOL_COST)
    np.testing.assert_allclose(costs[3], ref[3], rtol=RTOL_COST, atol=atol1)


def _assert_stats(stats, ref, n):
    for key in KEYS:
        np.testing.assert_allclose(stats[key], ref[key], rtol=2e-5, atol=1e-6 * np.abs(ref[key]).max(), err_msg=key)
    np.testing.assert_allclose(stats["post"].sum(), n, rtol=1e-6)
    for k in range(stats["obs*obs.T"].shape[0]):      # one accumulator is written to both mirrored slots
        assert np.array_equal(stats["obs*obs.T"][k], stats["obs*obs.T"][k].T), k


def _stencil_entries(H, W, diag):
    """adjacency entries of the complete 8-neighbour stencil on an H x W block (diagonal: the upper triangle i <= j)"""
    ii, jj = np.divmod(np.arange(H * W), W)
    inside = lambda i, j: (i >= 0) & (i < H) & (j >= 0) & (j < W) & ((i <= j) if diag else True)
    own = inside(ii, jj)
    return int(sum(np.count_nonzero(own & inside(ii + di, jj + dj)) for di in (-1, 0, 1) for dj in (-1, 0, 1) if di or dj))


class _Case:
    """inputs as the device holds them and the float64 reference of one case"""

    def __init__(self, S, K, form, beta, et, X, eid, w, geom, lp, labels):
        self.S, self.K, self.form, self.n, self.beta, self.et = S, K, form, len(X), beta, et
        self.X, self.eid, self.w, self.geom, self.lp, self.labels = X, eid, w, geom, lp, labels
        self.deg = np.bincount(eid.ravel(), minlength=self.n) if len(eid) else np.zeros(self.n, dtype=np.int64)
        self.D = max(4, (int(self.deg.max()) + 3) // 4 * 4)          # the adjacency width set_graph must find
        self.post, self.costs, self.stats = P.posteriors_costs_stats(labels, lp, X, eid, w, beta, et)
        self.atol1 = _cost1_atol(labels, eid, w, K, beta, et)

    def relabelled(self, labels):
        return _Case(self.S, self.K, self.form, self.beta, self.et, self.X, self.eid, self.w, self.geom, self.lp, labels)

    def block(self):
        b = _block(self.n, self.S, self.K)
        b.set_observations(self.X)
        b.set_graph(self.eid, self.w)
        assert b.get_adjacency()[0].shape[1] == self.D
        if self.form.startswith("grid"):
            # the launcher takes the grid form of the kernel (neighbours by geometry, weights from the forward-edge
            # records) only for eight-wide rows and an edge list that holds every edge of the stencil; the two forms
            # agree bit for bit, so no output tells them apart: what is asserted here is the launcher's condition
            assert self.D == 8 and 2 * len(self.eid) == _stencil_entries(*self.geom)
            b.set_grid(self.geom[0], self.geom[1], self.geom[2], 8)
        b.set_logprob(self.lp)
        b.set_labels(self.labels)
        return b

    def check(self, b, deterministic=False):
        """the call with posteriors against the reference; the statistics-only call against the call with posteriors"""
        stats, costs, post = b.posterior_stats(self.beta, self.et, want_posteriors=True)
        print("n=%d K=%d S=%d %s: post err %.2e, cost abs err %s of rtol * |ref| + atol %s" % (
            self.n, self.K, self.S, self.form, np.max(np.abs(post - self.post)), np.array2string(np.abs(costs - self.costs), precision=2),
            np.array2string(RTOL_COST * np.abs(self.costs) + np.array([0.0, self.atol1, 0.0, self.atol1]), precision=2)))
        assert np.max(np.abs(post - self.post)) < 2e-5
        _assert_stats(stats, self.stats, self.n)
        _assert_costs(costs, self.costs, self.atol1)
        stats2, costs2, none = b.posterior_stats(self.beta, self.et)
        assert none is None
        if deterministic:
            assert all(np.array_equal(stats2[key], stats[key]) for key in KEYS) and np.array_equal(costs2, costs)
        else:
            for key in KEYS:
                np.testing.assert_allclose(stats2[key], stats[key], rtol=1e-9, err_msg=key)
            np.testing.assert_allclose(costs2, costs, rtol=1e-9)
        return stats, costs, post


@functools.lru_cache(maxsize=4)             # (a case used twice in a row is built once)
def _case(S, K, form, n, beta, et, mode):
    rng = np.random.default_rng(1000 * S + 10 * K + FORMS.index(form) + n)
    X = _observations(rng, n, S)
    eid, w, geom = _graph(rng, form, n, X)
    lp = _f32(rng.normal(0.0, 3.0, (n, K)) - 5.0)
    return _Case(S, K, form, beta, et, X, eid, w, geom, lp, _labels(rng, mode, lp))


# ---- (a) the form matrix ---------------------------------------------------------------------------------------------
K_CYCLE = (1, 2, 3, 7, 16, 17, 20, 33, 64)
N_SPECS = ("1", "63", "64", "65", "TB-1", "TB", "TB+1", "2TB+1", "big")
BETAS = (0.0, 0.3, 1.3, 6.0)
MODES = ("random", "argmax", "one", "absent")
DIAG_N = {"63": 55, "64": 66, "65": 66, "TB-1": {128: 120, 256: 253}, "TB": {128: 136, 256: 276}, "TB+1": {128: 136, 256: 276},
          "2TB+1": {128: 276, 256: 528}, "big": 2485}          # triangular numbers next to the edge (N = 10, 11, 15, 16, 22, 23, 32, 70)


def _nodes(spec, form, TB):
    """the node count of a size class for an adjacency form, or None where the form has no block of that class"""
    n = {"1": 1, "63": 63, "64": 64, "65": 65, "TB-1": TB - 1, "TB": TB, "TB+1": TB + 1, "2TB+1": 2 * TB + 1, "big": 3080}[spec]
    if form == "grid_diag":
        d = DIAG_N.get(spec)
        return d[TB] if isinstance(d, dict) else d
    if form in ("grid_rect", "explicit8"):
        return n if _rect(n) else None                 # (1, 127 and 257 are no H x W with H >= 2)
    if form == "deg12" and n < 63:
        return None                                    # (too few nodes for a row of twelve)
    return n


def _form_matrix():
    cases, i = [], 0
    for S in range(1, 9):
        for f, form in enumerate(FORMS):
            K = K_CYCLE[i % 9]
            TB = tile_rows(K, S)[0]
            j = i + i // 9
            while _nodes(N_SPECS[j % 9], form, TB) is None:
                j += 1
            cases.append((S, K, form, _nodes(N_SPECS[j % 9], form, TB), BETAS[(i + i // 4) % 4], (i + i // 16) % 4,
                          MODES[(i + i // 4 + i // 16) % 4]))
            i += 1
    # the kernel's corner and the size below it (128-row tiles at the largest LDS share), on an edge of that tile
    cases += [(8, 64, "explicit8", 129, 1.3, 3, "argmax"), (8, 56, "grid_rect", 255, 1.3, 3, "argmax"), (8, 64, "grid_diag", 136, 0.3, 0, "random"),
              (5, 64, "ragged4", 127, 1.3, 3, "random"), (3, 64, "deg12", 257, 6.0, 3, "absent"), (7, 40, "isolated", 257, 1.3, 2, "argmax"),
              (4, 64, "grid_rect", 128, 0.3, 0, "one"), (6, 5, "ragged4", 1, 1.3, 3, "random"), (2, 6, "isolated", 1, 0.3, 1, "random")]
    return cases


FORM_CASES = _form_matrix()
