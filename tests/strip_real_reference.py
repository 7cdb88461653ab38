"""Float64 reference for the strip moves on REAL-VALUED problems (tests/test_strip_real_cpu.py, tests/test_gpu_strip_real.py).

The strips of one pass do not interact: bands are separated by a fixed row and segments by a fixed column, so no edge
joins two strips.  The strip kernels (strip.hip) can therefore be held to the exact optimum STRIP BY STRIP: after a pass,
every strip's labelling must cost no more, in float64, than what oracle/mrf_moves.strip_fusion reaches on that strip from
the same start, up to an allowance for the kernels' f32 arithmetic that is derived below and not fitted.

Everything here is NumPy on the CPU.  The three mutants at the end are move models that are wrong on purpose: the CPU test
shows that the per-strip check catches each of them on every case of the GPU matrix.
"""
import collections

import numpy as np

from oracle import mrf_moves as M
from oracle import ref_numpy as R
from oracle import synth
from tests.test_peel_filter import _problem

U32 = 2.0 ** -24          # unit roundoff of f32
OFFSET = 1024.0           # what the 'offset' family adds to every unary


def f32(x):
    """to f32 and back: the value the device stores"""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ per-strip quantities
def strip_ids(H, W, diagonal, orient, sr, sc):
    """-> sid[n]: the strip of each node on the cut (orient, sr, sc), -1 for the rim (the fixed rows and columns)"""
    nodes, _ = M.strip_node_table(H, W, diagonal, orient, sr, sc)
    n = H * (H + 1) // 2 if diagonal else H * W
    sid = -np.ones(n, dtype=np.int64)
    ss, pp = np.nonzero(nodes >= 0)
    sid[nodes[ss, pp]] = ss
    return sid


def _n_strips(sid):
    return int(sid.max()) + 1 if sid.size else 0


def _edge_strip(sid, eid):
    """-> the strip each edge belongs to (-1: both ends on the rim); no edge has its ends in two strips"""
    sa, sb = sid[eid[:, 0]], sid[eid[:, 1]]
    assert not np.any((sa >= 0) & (sb >= 0) & (sa != sb)), "an edge joins two strips"
    return np.maximum(sa, sb)


def strip_energies(sid, eid, w, unary, beta, labels):
    """-> e[NS]: per strip, the unaries of its nodes plus beta w_ij [l_i != l_j] over every undirected edge with an end in it"""
    NS = _n_strips(sid)
    lab = np.asarray(labels, dtype=np.int64)
    ins = sid >= 0
    e = np.bincount(sid[ins], weights=unary[np.nonzero(ins)[0], lab[ins]], minlength=NS)
    es = _edge_strip(sid, eid)
    k = es >= 0
    cut = (lab[eid[:, 0]] != lab[eid[:, 1]])[k]
    return e + np.bincount(es[k], weights=beta * w[k] * cut, minlength=NS)


def strip_allowance(sid, eid, w, unary, beta, labels, prop):
    """-> a[NS], the f32 rounding allowance of a strip's binary problem {keep l_i, take p_i}:

        a_s = 12 (T_s + 6) u M_s,    u = 2^-24,
        T_s = cells of the strip,    M_s = sum_{i in s} ( max(|u_i(l_i)|, |u_i(p_i)|) + beta sum_j w_ij ).

    Derivation (the textbook forward bound of a running sum, nothing measured): the DP adds, per cell and path, the cell's
    cost and at most four pair terms to the running minimum and takes over one predecessor: at most 6 f32 additions per
    step, each with a relative error of at most u on a partial sum.  No partial sum of a path exceeds M_s in magnitude:
    M_s is the sum of the largest cost every cell can contribute, i.e. the largest value a DP entry can reach.  The walk
    takes T_s steps through the strip and 6 more through the keep-only cells behind it, so the cost the DP holds for one
    path differs from that path's exact cost by at most 6 (T_s + 6) u M_s.  The kernel decides between labellings by
    comparing two such sums, so the labelling it returns can cost at most 12 (T_s + 6) u M_s more than the exact optimum --
    and, the current labelling being one of the paths, at most that much more than the current one."""
    NS = _n_strips(sid)
    n = len(sid)
    wtot = np.bincount(eid[:, 0], weights=w, minlength=n) + np.bincount(eid[:, 1], weights=w, minlength=n)
    ar = np.arange(n)
    big = np.maximum(np.abs(unary[ar, np.asarray(labels, dtype=np.int64)]), np.abs(unary[ar, np.asarray(prop, dtype=np.int64)]))
    ins = sid >= 0
    T = np.bincount(sid[ins], minlength=NS)
    Ms = np.bincount(sid[ins], weights=(big + beta * wtot)[ins], minlength=NS)
    return 12.0 * (T + 6) * U32 * Ms


def alternative_costs(g, unary, labels, beta):
    """-> (cost[n, K] of every label as a node's proposal, +inf at its own label; bound[n, K]): label k of node i is as
    good a proposal as the best one k1, as far as f32 can tell, when cost[i, k] - cost[i, k1] < bound[i, k], with
    bound[i, k] = 8 u (|u_i(k1)| + |u_i(k)| + beta sum_j w_ij): propose_grid_kernel forms each cost by at most eight f32
    subtractions from the unary term"""
    K = unary.shape[1]
    ar = np.arange(g.n)
    cost = unary - beta * M.neighbour_hist(g, labels, K)
    cost[ar, labels] = np.inf
    k1 = np.argmin(cost, axis=1)
    bound = 8.0 * U32 * (np.abs(unary[ar, k1])[:, None] + np.abs(unary) + beta * g.wtot[:, None])
    return cost, bound


def ambiguous_proposals(g, unary, labels, beta):
    """-> bool[n]: the f64 costs of the node's best and second-best alternative label differ by less than
    8 u (|u_i(k1)| + |u_i(k2)| + beta sum_j w_ij): the device's f32 proposal may differ from M.best_alternative there"""
    cost, bound = alternative_costs(g, unary, labels, beta)
    if cost.shape[1] < 3:
        return np.zeros(g.n, dtype=bool)
    ar = np.arange(g.n)
    order = np.argsort(cost, axis=1, kind="stable")
    k1, k2 = order[:, 0], order[:, 1]
    return cost[ar, k2] - cost[ar, k1] < bound[ar, k2]


# ------------------------------------------------------------------------------------------------ problems
Problem = collections.namedtuple("Problem", "n H W K diagonal beta eid w unary init extra")


def start_labels(seed, n, K, truth_noisy, start):
    """'noisy': the truth with 5 % noise (a warm E-step);  'random': a uniformly random labelling, so that the DP, not
    the filter, decides most strips"""
    if start == "noisy":
        return truth_noisy.astype(np.int64)
    assert start == "random"
    return np.random.default_rng(seed + 1000).integers(0, K, n).astype(np.int64)


def make_problem(family, seed, H, W, K, diagonal, beta, start="noisy"):
    """The three input families, every input cast to f32 and back so that the model reads what the device stores.
    real:      the real-valued recipe of tests/test_peel_filter._problem (gamma unaries, weights exp(-d / 2))
    offset:    real with 1024 added to every unary: the same optimum, far larger magnitudes in the raw-cost DP
    emission:  a synthetic block of oracle/synth with 2 % of the observations multiplied by 5, unary = -log density: the
               outlier bins of a fit, whose unaries reach 1e2 .. 1e3.  extra = (X, means, covars): the GPU test runs
               the emission kernel on them and reads the unaries back from the block."""
    if family in ("real", "offset"):
        n, eid, w, un, lab = _problem(seed, H, W, K, diagonal, integer=False)
        if family == "offset":
            un = f32(un) + OFFSET
        extra = None
    else:
        assert family == "emission"
        blk = synth.make_block(seed=seed, H=H, W=W, S=4, K=K, diagonal=diagonal, mean_run=6)
        rng = np.random.default_rng(seed + 500)
        X = blk["X"].copy()
        n = X.shape[0]
        X[rng.random(n) < 0.02] *= 5.0
        X = f32(X)
        w, eid = R.edge_weights_from_distance(R.grid_edges(X, H, W, diagonal, 8), 0.5)
        un = -R.log_multivariate_normal_density_full(X, blk["means"], blk["covars"])
        truth = blk["labels_true"].astype(np.int64)
        lab = np.where(rng.random(n) < 0.05, rng.integers(0, K, n), truth)
        extra = (X, blk["means"], blk["covars"])
    return Problem(n, H, W, K, diagonal, float(beta), np.int64(eid), f32(w), f32(un), start_labels(seed, n, K, lab, start), extra)


# ------------------------------------------------------------------------------------------------ move models
def _fusion(p, g, lab, prop, orient, sr, sc):
    out = np.asarray(lab, dtype=np.int64).copy()
    M.strip_fusion(g, p.unary, out, prop, p.beta, p.H, p.W, p.diagonal, orient, sr, sc)
    return out


def _proposal(p, g, lab, alpha):
    return np.full(p.n, alpha, dtype=np.int64) if alpha >= 0 else M.best_alternative(g, p.unary, lab, p.beta)


def model_pass(p, g, lab, orient, sr, sc, alpha):
    """the exact move: alpha >= 0 the strip expansion of alpha, alpha < 0 the fusion with every node's best alternative"""
    return _fusion(p, g, lab, _proposal(p, g, lab, alpha), orient, sr, sc)


def _is_antidiagonal(p, eid):
    ii, jj = M.grid_coords(p.H, p.W, p.diagonal)
    a, b = eid[:, 0], eid[:, 1]
    return (ii[b] - ii[a]) * (jj[b] - jj[a]) == -1


def mutant_no_antidiagonal(p, g, lab, orient, sr, sc, alpha):
    """(a) wrong on purpose: the DP ignores the anti-diagonal weights inside a strip (one weight family dropped)"""
    sid = strip_ids(p.H, p.W, p.diagonal, orient, sr, sc)
    inside = (sid[p.eid[:, 0]] >= 0) & (sid[p.eid[:, 0]] == sid[p.eid[:, 1]])
    gm = M.Graph(p.n, p.eid, np.where(inside & _is_antidiagonal(p, p.eid), 0.0, p.w))
    return _fusion(p, gm, lab, _proposal(p, g, lab, alpha), orient, sr, sc)


def mutant_no_rim(p, g, lab, orient, sr, sc, alpha):
    """(b) wrong on purpose: the DP ignores the edges from a strip cell to the rim"""
    sid = strip_ids(p.H, p.W, p.diagonal, orient, sr, sc)
    to_rim = (sid[p.eid[:, 0]] >= 0) != (sid[p.eid[:, 1]] >= 0)
    gm = M.Graph(p.n, p.eid, np.where(to_rim, 0.0, p.w))
    return _fusion(p, gm, lab, _proposal(p, g, lab, alpha), orient, sr, sc)


def mutant_half_cap(p, g, lab, orient, sr, sc, alpha):
    """(c) wrong on purpose: the filter in front of an expansion with its cap halved (M.peel with disc / 2), the DP allowed
    only on what that filter leaves.  M.peel keeps node i while s_i <= cap_i, with s_i = u_i(alpha) - u_i(l_i) + pair_i;
    halving disc is the test 2 s_i <= cap_i, which M.peel makes on unaries whose difference is 2 (u_i(alpha) - u_i(l_i)) +
    pair_i (it adds the second pair_i itself).  (The fusion pass has no model of its filter: there this is the exact move.)"""
    lab = np.asarray(lab, dtype=np.int64)
    if alpha < 0:
        return model_pass(p, g, lab, orient, sr, sc, alpha)
    ar = np.arange(p.n)
    li, lj = lab[g.src], lab[g.col]
    pair = np.zeros(p.n)
    np.add.at(pair, g.src, p.beta * g.wgt * ((lj != alpha).astype(np.float64) - (lj != li)))
    un2 = np.zeros_like(p.unary)
    un2[:, alpha] = 2.0 * (p.unary[:, alpha] - p.unary[ar, lab]) + pair
    un2[ar, lab] = 0.0
    U, _ = M.peel(g, un2, lab, p.beta, p.H, p.W, p.diagonal, orient, sr, sc, alpha)
    return _fusion(p, g, lab, np.where(U, alpha, lab), orient, sr, sc)


MUTANTS = {"no anti-diagonal": mutant_no_antidiagonal, "no rim": mutant_no_rim, "half cap": mutant_half_cap}


# ------------------------------------------------------------------------------------------------ the check of one pass
class PassCheck(object):
    """One pass (orient, cut, alpha; alpha < 0: fusion) from the labelling L0: L1 is the labelling under test, L* the exact
    move's.  Holds the per-strip float64 energies e0, e1, es, the allowance a, and which strips hold an ambiguous proposal."""

    def __init__(self, p, g, L0, L1, orient, sr, sc, alpha, Ls=None, count=None):
        self.orient, self.cut, self.alpha, self.count = orient, (sr, sc), alpha, count
        self.L0, self.L1 = np.asarray(L0, dtype=np.int64), np.asarray(L1, dtype=np.int64)
        self.Ls = model_pass(p, g, self.L0, orient, sr, sc, alpha) if Ls is None else Ls
        self.sid = sid = strip_ids(p.H, p.W, p.diagonal, orient, sr, sc)
        NS = _n_strips(sid)
        self.cells = np.bincount(sid[sid >= 0], minlength=NS)
        self.moved = self.L1 != self.L0
        ref_prop = _proposal(p, g, self.L0, alpha)
        self.amb = np.zeros(NS, dtype=bool)
        self.bad_label = np.zeros(p.n, dtype=bool)        # (iii): a changed node took something that is no proposal of its
        mv = np.nonzero(self.moved)[0]
        if alpha >= 0:
            self.bad_label[mv] = self.L1[mv] != alpha
        else:
            cost, bound = alternative_costs(g, p.unary, self.L0, p.beta)
            self.bad_label[mv] = ~(cost[mv, self.L1[mv]] - cost[mv, ref_prop[mv]] < bound[mv, self.L1[mv]])
            self.bad_label[mv] &= self.L1[mv] != ref_prop[mv]
            nodes = ambiguous_proposals(g, p.unary, self.L0, p.beta) & (sid >= 0)
            self.amb[np.unique(sid[nodes])] = True
        self.prop = prop = np.where(self.moved, self.L1, ref_prop)       # what every node kept or took
        self.e0, self.e1, self.es = (strip_energies(sid, p.eid, p.w, p.unary, p.beta, L) for L in (self.L0, self.L1, self.Ls))
        self.a = strip_allowance(sid, p.eid, p.w, p.unary, p.beta, self.L0, prop)

    def name(self):
        return "orient %d cut %s %s" % (self.orient, self.cut, "fusion" if self.alpha < 0 else "label %d" % self.alpha)

    def _rows(self, strips):
        return "; ".join("strip %d (%d cells): e(L0) %.9g  e(L1) %.9g  e(L*) %.9g  allowance %.3g"
                         % (s, self.cells[s], self.e0[s], self.e1[s], self.es[s], self.a[s]) for s in strips[:6])

    def failures(self, scale=1.0):
        """-> the violated assertions as text (empty: the pass holds); `scale` multiplies the allowance (0: exact arithmetic)"""
        out = []
        up = np.nonzero(self.e1 > self.e0 + scale * self.a)[0]
        if len(up):
            out.append("(i) %s raises %d strips: %s" % (self.name(), len(up), self._rows(up)))
        lost = np.nonzero((self.e1 > self.es + scale * self.a) & ~self.amb)[0]
        if len(lost):
            out.append("(ii) %s misses the optimum on %d strips: %s" % (self.name(), len(lost), self._rows(lost)))
        if np.any(self.moved & (self.sid < 0)):
            out.append("(iii) %s moves %d rim nodes" % (self.name(), int((self.moved & (self.sid < 0)).sum())))
        if self.bad_label.any():
            i = int(np.nonzero(self.bad_label)[0][0])
            out.append("(iii) %s: %d nodes took a label that is not their proposal (node %d: %d -> %d)"
                       % (self.name(), int(self.bad_label.sum()), i, self.L0[i], self.L1[i]))
        if self.count is not None and self.count != int(self.moved.sum()):
            out.append("(iv) %s reports %d changes, %d labels differ" % (self.name(), self.count, int(self.moved.sum())))
        return out

    def misses(self, scale=1.0):
        """strips on which (ii) fails"""
        return int(np.sum((self.e1 > self.es + scale * self.a) & ~self.amb))

    def excess_ratio(self, a=None):
        """max over the unambiguous strips of (e(L1) - e(L*)) / allowance (<= 1 is what (ii) asserts)"""
        a = self.a if a is None else a
        ok = ~self.amb & (self.cells > 0)
        return float(np.max((self.e1 - self.es)[ok] / a[ok])) if ok.any() else 0.0

    def same_as_model(self):
        """-> (strips whose labelling is exactly the model's, unambiguous strips with cells)"""
        ok = ~self.amb & (self.cells > 0)
        diff = np.zeros(len(self.cells), dtype=bool)
        d = (self.L1 != self.Ls) & (self.sid >= 0)
        diff[np.unique(self.sid[d])] = True
        return int((ok & ~diff).sum()), int(ok.sum())


def sequence(case_passes, labels):
    """the passes of one entry: 'expansion' -> every listed label on every (orient, cut); 'fusion' -> one pass per cut"""
    exp = [(orient, sr, sc, a) for orient, (sr, sc) in case_passes for a in labels]
    fus = [(orient, sr, sc, -1) for orient, (sr, sc) in case_passes]
    return {"expansion": exp, "fusion": fus}


def run_sequence(p, g, passes, step, memo=None):
    """Carries the labelling of `step(L0, orient, sr, sc, alpha) -> (L1, count or None)` forward through `passes`, starting
    at p.init -> [PassCheck].  `memo` (a dict) keeps the exact move per (pass, L0): entries that reach the same labelling
    share it."""
    lab = p.init.copy()
    out = []
    for orient, sr, sc, alpha in passes:
        L1, count = step(lab, orient, sr, sc, alpha)
        Ls = None
        if memo is not None:
            key = (orient, sr, sc, alpha, lab.tobytes())
            if key not in memo:
                memo[key] = model_pass(p, g, lab, orient, sr, sc, alpha)
            Ls = memo[key]
        out.append(PassCheck(p, g, lab, L1, orient, sr, sc, alpha, Ls, count))
        lab = np.asarray(L1, dtype=np.int64).copy()
    return out


# ------------------------------------------------------------------------------------------------ the matrix
Case = collections.namedtuple("Case", "family seed H W K diagonal beta start passes labels")

CUT_A = ((0, (0, 0)), (1, (3, 17)), (0, (5, 63)))      # the three cuts, orientations alternating ...
CUT_B = ((1, (0, 0)), (0, (3, 17)), (1, (5, 63)))      # ... and the other way round
K64_LABELS = (0, 7, 21, 31, 32, 40, 62, 63)


def _case(family, seed, H, W, K, diagonal, beta, start="noisy", passes=CUT_A, labels=None):
    return Case(family, seed, H, W, K, diagonal, beta, start, passes, tuple(range(K)) if labels is None else labels)


def case_id(c):
    return "%s-%dx%d%s-K%d-b%g-%s-s%d" % (c.family, c.H, c.W, "tri" if c.diagonal else "", c.K, c.beta, c.start, c.seed)


# Shapes: one segment and two (W = 64 + 6, 2 * 64 + 3), a band that is all of the block (H = 7), upper-triangular blocks below
# and at the segment length; K = 4, 8, 20 and the 64-label kernel form; the three betas and cuts dealt over them.  The K = 20
# case runs two of the cuts and has the smallest shape with a full segment: the model costs 0.1 s per pass whatever the size.  The seeds were chosen on the CPU (tests/test_strip_real_cpu.py
# states what they have to give); as it happened the first seeds tried gave it.
CASES = [
    _case("real", 3, 12, 20, 4, False, 0.75),
    _case("real", 3, 23, 70, 4, False, 0.75, passes=CUT_B),
    _case("real", 5, 12, 131, 8, False, 0.5),
    _case("real", 6, 7, 64, 20, False, 2.0, start="random", passes=(CUT_B[0], CUT_A[2])),
    _case("real", 7, 41, 41, 8, True, 2.0, start="random"),
    _case("real", 8, 64, 64, 8, True, 0.5, passes=CUT_B),
    _case("real", 9, 12, 40, 64, False, 0.75, labels=K64_LABELS),
    _case("emission", 10, 23, 70, 8, False, 0.5),
    _case("emission", 11, 41, 41, 4, True, 0.75, passes=CUT_B),
    _case("offset", 3, 12, 20, 4, False, 0.75),
    _case("offset", 3, 23, 70, 4, False, 2.0, passes=CUT_B),
]

def weights_from_adjacency(nbr, wgt, eid):
    """the weight the block stores for each edge of eid, from its adjacency rows (nbr[n, D], wgt[n, D]; -1: no neighbour)"""
    n, D = nbr.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), D)
    cols = nbr.reshape(-1).astype(np.int64)
    ok = cols >= 0
    keys = rows[ok] * n + cols[ok]
    order = np.argsort(keys)
    keys, vals = keys[order], wgt.reshape(-1)[ok][order].astype(np.float64)
    q = eid[:, 0] * np.int64(n) + eid[:, 1]
    pos = np.searchsorted(keys, q)
    assert np.all(pos < len(keys)) and np.array_equal(keys[pos], q), "an edge of the list is not in the block's adjacency"
    return vals[pos]
