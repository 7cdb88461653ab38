"""TEST INFRASTRUCTURE ONLY -- inputs for the multi-label coarse sweep (solve.hip: coarse_sweep_nocount; coarse.hip) and
what the float64 move model (oracle/mrf_moves.coarse_sweep) makes of them.  tests/test_coarse_reference_cpu.py asserts every
case's precondition without a GPU; tests/test_gpu_coarse_sweep.py asserts it again and compares the kernels with the model.

Random sweeps (SWEEPS): the integer problems of tests/test_gpu_estep.py, from their random start, where a sweep that never
rebuilds ends in another labelling than the one-by-one sequence.

Constructed cases (REBUILDS, MIRROR, QUIET): once a labelling has had a few sweeps, a sweep that never rebuilds gives the
one-by-one labelling on almost every random input, so the sparse regime -- where the device-side gates actually skip work --
is built by hand.  All weights are 1/8, beta = 1, the start is the constant labelling 0, every node's unary terms are 0 for
label 0 and +20 for every other label except in the regions named below; all super-cells named are whole ones.

  A   one super-cell that takes label 1: label 1 at -30 per node.
  B   the super-cell next to A; label 1 at +20 (label 1 leaves its nodes alone), label 2 at d / |B| per node with
      d = -(w_B - w_AB / 2), w_B the weight of all edges that leave B and w_AB of those between A and B.  B alone switches to
      label 2 for d + w_B - [A carries label 1] w_AB (the boundary to A is paid for already once A has moved):
          d + w_B = +w_AB / 2 >= 0 > d + w_B - w_AB = -w_AB / 2
      so B moves only in a problem that knows A's move, and only if that knowledge crossed from A's super-cell into B's.
  T   a super-cell in A's wavefront, away from both: label 1 at -30, label 2 at -20.  From the labelling 0 label 2 takes
      it (and the apply pass would overwrite the 1 it has by then); from the labelling label 1 left, label 2 costs +10 a node.
"""
import functools

import numpy as np

from oracle import mrf_moves as M
from oracle import ref_numpy as R
from tests.test_gpu_estep import _integer_problem

BETA = 1.0
WEIGHT = 0.125


# ------------------------------------------------------------------------------------------------ random sweeps
# (label sets: batches of 1, 2, 3 and 4 labels, a full batch and a partial one, two full batches and one, a mask with gaps)
LABEL_SETS = [(2, None), (3, None), (4, None), (5, None), (7, None), (9, None), (9, (0, 3, 4, 8))]
# H, W, diagonal, then three (scale, offset, shift_r, shift_c): the first is the sweep with the precondition, the others
# follow on the same block (other offsets and cuts: child blocks, flag and counters are used again)
SWEEP_SHAPES = [
    (20, 70, False, [(2, 1, 0, 0), (4, 2, 3, 17), (2, 0, 5, 63)]),
    (40, 40, True, [(2, 0, 1, 7), (2, 1, 4, 40), (4, 1, 2, 21)]),
    (24, 130, False, [(4, 3, 2, 40), (4, 0, 0, 5), (2, 1, 3, 62)]),
    (40, 136, False, [(8, 5, 0, 0), (8, 2, 5, 33), (4, 3, 1, 1)]),
]
SWEEPS = [(H, W, diag, K, labels, tuple(steps)) for (H, W, diag, steps) in SWEEP_SHAPES for (K, labels) in LABEL_SETS]


def sweep_id(case):
    H, W, diag, K, labels, steps = case
    return "%dx%d%s-s%do%d-K%d%s" % (H, W, "tri" if diag else "", steps[0][0], steps[0][1], K,
                                      "" if labels is None else "-mask" + "".join(str(a) for a in labels))


def per_label(K, alphas, counts):
    out = np.zeros(K, dtype=np.int64)
    out[list(alphas)] = counts
    return out


@functools.lru_cache(maxsize=None)
def sweep_model(case):
    """-> dict: the problem, `stale` = the labelling of the first sweep without rebuilds, and per sweep (labels after,
    changed per label) of the one-by-one model.  Computed once; the arrays are shared and must not be written."""
    H, W, diag, K, labels, steps = case
    n, eid, w, lp, init = _integer_problem(21 + K, H, W, K, diag)
    g = M.Graph(n, eid, w)
    alphas = list(range(K)) if labels is None else list(labels)
    s, off, sr, sc = steps[0]
    stale = init.astype(np.int64).copy()
    M.coarse_sweep(g, -lp, stale, BETA, H, W, diag, s, off, alphas, sr, sc, stale=True)
    lab = init.astype(np.int64).copy()
    after = []
    for (s, off, sr, sc) in steps:
        cnt = M.coarse_sweep(g, -lp, lab, BETA, H, W, diag, s, off, alphas, sr, sc)
        after.append((lab.copy(), per_label(K, alphas, cnt)))
    for a, _ in after:
        a.setflags(write=False)
    return dict(n=n, eid=eid, w=w, lp=lp, init=init, alphas=alphas, stale=stale, after=after)


# ------------------------------------------------------------------------------------------------ constructed cases
class Constructed(object):
    def __init__(self, name, H, W, diagonal, K, scale, off, labels, cut):
        self.name, self.H, self.W, self.diagonal, self.K = name, H, W, diagonal, K
        self.scale, self.off, self.labels, self.cut = scale, off, tuple(labels), cut
        self.n = H * (H + 1) // 2 if diagonal else H * W
        e = R.grid_edges(np.ones((self.n, 2)), H, W, diagonal, 8)
        self.eid = np.int64(e[:, :2])
        self.w = np.full(len(self.eid), WEIGHT)
        self.un = np.full((self.n, K), 20.0)
        self.un[:, 0] = 0.0
        self.init = np.zeros(self.n, dtype=np.int64)
        self.B = None                                   # nodes of super-cell B
        ii, jj = M.grid_coords(H, W, diagonal)
        self._cell = ((ii + off) // scale) * 100000 + (jj + off) // scale

    @property
    def lp(self):
        return -self.un

    def cell(self, I, J):
        nodes = np.flatnonzero(self._cell == I * 100000 + J)
        assert len(nodes) == self.scale ** 2, (self.name, I, J, len(nodes))        # a whole super-cell
        return nodes

    def cross_weight(self, nodes, other=None):
        """weight of the edges with exactly one end in `nodes` (other: and the other end in `other`)"""
        inn = np.zeros(self.n, dtype=bool)
        inn[nodes] = True
        a, b = self.eid[:, 0], self.eid[:, 1]
        m = inn[a] != inn[b]
        if other is not None:
            ino = np.zeros(self.n, dtype=bool)
            ino[other] = True
            m &= (ino[a] | ino[b])
        return float(self.w[m].sum())

    def model(self, stale=False):
        """-> (labels, changed per label) of the sweep under the move model"""
        g = M.Graph(self.n, self.eid, self.w)
        lab = self.init.copy()
        cnt = M.coarse_sweep(g, self.un, lab, BETA, self.H, self.W, self.diagonal, self.scale, self.off, list(self.labels),
                             self.cut[0], self.cut[1], stale=stale)
        return lab, per_label(self.K, self.labels, cnt)


def _rebuild_case(diagonal, scale, off, place, labels, cut):
    """A | B across a wavefront's column boundary of the coarsen pass (thread column j + off = 63 | 64: 'wave'), across a
    workgroup's (255 | 256: 'group'), or in consecutive coarse rows (A 'above' / 'below' B)."""
    s = scale
    if place in ("wave", "group"):
        edge = 64 if place == "wave" else 256
        A, B, T = (1, edge // s - 1), (1, edge // s), (1, edge // s - 5)
        W = edge + 3 * s + 1
    else:
        A, B = ((1, 6), (2, 6)) if place == "above" else ((2, 6), (1, 6))
        T = (A[0], 11)
        W = 14 * s + 1
    H = W if diagonal else 5 * s + 1
    c = Constructed("%s-s%do%d-%s" % ("tri" if diagonal else "rect", s, off, place), H, W, diagonal, 4, s, off, labels, cut)
    a, b, t = c.cell(*A), c.cell(*B), c.cell(*T)
    c.un[a, 1] = -30.0
    w_b, w_ab = c.cross_weight(b), c.cross_weight(b, a)
    assert w_ab > 0
    c.un[b, 2] = -(w_b - 0.5 * w_ab) / len(b)
    c.un[t, 1] = -30.0
    c.un[t, 2] = -20.0
    c.A, c.B, c.T = a, b, t
    c.d_plus_wb, c.w_ab = 0.5 * w_ab, w_ab
    return c


_PLACES = ["wave", "group", "above", "below"]
# (the label sets: label 1 first in a batch of two and of three; behind label 0, which moves nothing, in a batch of four)
_LABELS = {"wave": (1, 2, 3), "group": (0, 1, 2, 3), "above": (1, 2), "below": (1, 2, 3)}
_GEOM = [(False, 2, 1), (False, 4, 3), (True, 2, 0), (True, 4, 1)]
_CUTS = {"wave": (0, 0), "group": (2, 40), "above": (1, 7), "below": (4, 21)}
REBUILD_IDS = ["%s-s%do%d-%s" % ("tri" if d else "rect", s, o, p) for (d, s, o) in _GEOM for p in _PLACES]


@functools.lru_cache(maxsize=None)
def rebuild_case(name):
    for (d, s, o) in _GEOM:
        for p in _PLACES:
            if "%s-s%do%d-%s" % ("tri" if d else "rect", s, o, p) == name:
                return _rebuild_case(d, s, o, p, _LABELS[p], _CUTS[p])
    raise KeyError(name)


MIRROR_IDS = ["rect-s2o1", "tri-s4o1"]


@functools.lru_cache(maxsize=None)
def mirror_case(name):
    """label 1 moves nothing, labels 2 and 3 move one super-cell each, far apart: the batch's flag is down at the rebuild of
    label 2 and up at the rebuild of label 3, and the rebuilt numbers are the ones of the batch's start where it matters."""
    diagonal, s, off = {"rect-s2o1": (False, 2, 1), "tri-s4o1": (True, 4, 1)}[name]
    W = 64 + 3 * s + 1
    H = W if diagonal else 5 * s + 1
    c = Constructed("mirror-" + name, H, W, diagonal, 4, s, off, (1, 2, 3), (3, 11))
    c.un[c.cell(1, 4), 2] = -30.0
    c.un[c.cell(2, 64 // s), 3] = -30.0
    return c


@functools.lru_cache(maxsize=None)
def quiet_case(name):
    """no label switches any super-cell: every gate stays down"""
    diagonal, s, off = {"rect-s2o1": (False, 2, 1), "tri-s4o1": (True, 4, 1)}[name]
    W = 64 + 3 * s + 1
    H = W if diagonal else 5 * s + 1
    return Constructed("quiet-" + name, H, W, diagonal, 4, s, off, (0, 1, 2, 3), (0, 0))


# ------------------------------------------------------------------------------------------------ strided rows
STRIDED = [(2, 1), (4, 1)]          # (scale, offset) on the 8200 x 6 block


@functools.lru_cache(maxsize=None)
def strided_model(scale, off):
    """8200 x 6, K = 3: one column of workgroups, more coarse rows than the 2048 workgroups a rebuild or a gated apply pass
    gets -> (problem, labels after the full sweep, changed per label)"""
    H, W, K = 8200, 6, 3
    n, eid, w, lp, init = _integer_problem(31, H, W, K, False)
    g = M.Graph(n, eid, w)
    lab = init.astype(np.int64).copy()
    cnt = M.coarse_sweep(g, -lp, lab, BETA, H, W, False, scale, off, [0, 1, 2], 2, 9)
    lab.setflags(write=False)
    return dict(H=H, W=W, K=K, n=n, eid=eid, w=w, lp=lp, init=init, after=lab, counts=per_label(K, [0, 1, 2], cnt), cut=(2, 9))


# ------------------------------------------------------------------------------------------------ the batched build
BUILD_K = 5
BUILD_OFFSETS = {2: (0, 1), 4: (0, 3), 8: (0, 5)}
BUILD_SHAPES = [(9, 9, True), (4, 5, False), (26, 70, False), (41, 41, True)]
# label 2: every node of one super-cell carries it; 3: absent from the labelling; 0 and K - 1.  By batch size:
BUILD_ALPHAS = {1: (2,), 2: (3, 0), 3: (0, 4, 2), 4: (4, 2, 3, 0)}


def build_problem(H, W, diagonal):
    """the integer problem with a labelling that has no label 3 and carries label 2 on rows 2..18 x columns 2..18 (with a
    whole super-cell inside at every scale and offset of BUILD_OFFSETS where the block is that large)"""
    n, eid, w, lp, init = _integer_problem(9, H, W, BUILD_K, diagonal)
    lab = init.astype(np.int64).copy()
    lab[lab == 3] = 1
    ii, jj = M.grid_coords(H, W, diagonal)
    lab[(ii >= 2) & (ii < 19) & (jj >= 2) & (jj < 19)] = 2
    return n, eid, w, lp, lab


REAL_BETA = 0.75


def real_problem():
    """synth.make_block, 60 x 60 upper triangle, K = 6: real-valued unary terms and weights -> (blk, eid, w, labels)"""
    from oracle import synth
    blk = synth.make_block(5, 60, 60, 4, 6, True)
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    n = blk["X"].shape[0]
    rng = np.random.default_rng(4)
    lab = np.where(rng.random(n) < 0.2, rng.integers(0, 6, n), blk["labels_true"]).astype(np.int64)
    return blk, eid, w, lab


def problem_with_bounds(eid, w32, un32, labels, beta, H, W, diagonal, s, off, alpha):
    """The float64 problem of f32 inputs (weights and unary terms as the device holds them) and how far an f32 sum in any
    order may lie from it: for every super-cell T * 2^-23 * sum |terms| over the terms the reference (mrf_moves.coarse_problem)
    adds into its D -- u_alpha - u_cur per node, beta t00 per inside edge, beta (t10 - t00 - lambda) resp.
    beta (t01 - t00 - lambda) per cross edge and end -- or into a lam slot -- lambda per cross edge of the pair; T counts the
    terms that are not zero (a zero adds no rounding), so a D or lam made of none or one of them has to be exact.
    -> (D, lam, bound_D[nc], bound_lam[nc, 4], threshold[nc] above which the kernel pins, bound_threshold[nc])"""
    n = un32.shape[0]
    g = M.Graph(n, eid, w32)
    D, lam, cnode, Hc, Wc = M.coarse_problem(g, un32, labels, beta, H, W, diagonal, s, off, alpha)
    nc = D.shape[0]
    lab = np.asarray(labels, dtype=np.int64)
    u = 2.0 ** -23
    T, A = np.zeros(nc), np.zeros(nc)

    def add(cells, terms):
        t = np.abs(terms)
        T[:] += np.bincount(cells[t > 0], minlength=nc)
        A[:] += np.bincount(cells, weights=t, minlength=nc)

    add(cnode, un32[np.arange(n), alpha] - un32[np.arange(n), lab])
    a, b = g.edge_ids[:, 0], g.edge_ids[:, 1]
    la, lb = lab[a], lab[b]
    t00, t01, t10 = g.w * (la != lb), g.w * (la != alpha), g.w * (alpha != lb)
    ca, cb = cnode[a], cnode[b]
    same = ca == cb
    add(ca[same], beta * t00[same])
    x = ~same
    lv = 0.5 * (t10[x] + t01[x] - t00[x])
    add(ca[x], beta * (t10[x] - t00[x] - lv))
    add(cb[x], beta * (t01[x] - t00[x] - lv))
    # the lam slots: the reference's own assignment
    ii, jj = M.grid_coords(H, W, diagonal)
    I, J = (ii + off) // s, (jj + off) // s
    dI, dJ = I[b[x]] - I[a[x]], J[b[x]] - J[a[x]]
    fwd = ~((dI == 0) & (dJ == -1))
    slot = np.where(dI == 0, 0, 2 + dJ)
    Tl, Al = np.zeros((nc, 4)), np.zeros((nc, 4))
    np.add.at(Tl, (ca[x][fwd], slot[fwd]), (lv[fwd] > 0) * 1.0)
    np.add.at(Al, (ca[x][fwd], slot[fwd]), lv[fwd])
    np.add.at(Tl, (cb[x][~fwd], 0), (lv[~fwd] > 0) * 1.0)
    np.add.at(Al, (cb[x][~fwd], 0), lv[~fwd])
    assert np.allclose(Al, lam, rtol=1e-12, atol=0) and lv.min() >= 0
    # the pin threshold (not a tolerance: the zone in which the pinned mask may differ): a sum of Tw weights, two products
    wcross = M.coarse_cross_weight(g, H, W, diagonal, s, off)
    Tw = np.bincount(ca[x], minlength=nc) + np.bincount(cb[x], minlength=nc)
    thr = beta * wcross * 1.0001 + 1e-6
    thr_bound = (Tw + 2) * u * thr
    return D, lam, T * u * A, Tl * u * Al, thr, thr_bound
