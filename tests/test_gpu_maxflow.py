"""GPU: one alpha-expansion of a general graph (csrc/maxflow.hip: lock-free push-relabel with global relabelling) against
the exact integer max-flow of tests/maxflow_reference.py.

LABEL FOR LABEL on dyadic problems.  w and lp are multiples of 1/64, beta is 0.5, 1 or 2 and the largest single term
(`top`) is forced to 128 -- by two extra nodes of equal label joined by one edge of weight 128 / beta (`with_anchor`), or by
one unary term of 128 -- so scale = 2^24 / top = 2^17 and every float32 product, sum, ceil and truncation of the kernels is
exact, whatever the summation order or the contraction of multiply-adds.  The device then solves the integer problem
`quantised_problem` builds, and the set it switches must be `kept_side`: the active nodes without a residual path to the
sink, which is the same for every maximum flow.  Every such test asserts that top is a power of two BEFORE it calls the
device (a precondition of the reference; no case is left out for it), then: the labels equal the reference node for node,
the returned count equals the number of labels that changed, a second call returns 0.

ENERGY on real-valued problems (seeded k-nearest-neighbour graphs, random initial labels), e in float64:
  e1 <= exact_expansion_energy + allowance   and   e1 <= e0 + allowance,
with the allowance of `maxflow_reference.expansion_allowance(got, best)`, derived there.  In short, with q = top / 2^24,
u = 2^-24, `got` the set the device switched and `best` the exact optimum (the empty set for the second bound):

  allowance =   sum over nodes only in got    r_i
              + sum over nodes only in best   (2 q + r_i)
              + sum over arcs cut by got only   (q + 4 u c_ij)  +  sum over arcs cut by best only   4 u c_ij  +  1e-13 |e0|
  r_i = u (|lp_i,alpha| + |lp_i,l| + (t_i + 1) max(|lp_i,l - lp_i,alpha|, |theta_i|) + 2 beta sum'_j w_ij + 2 |theta_i|)

(t_i, sum': the neighbours that enter theta_i).  top is the kernel's own, the largest single term; nothing is multiplied by
n or by the sum of all weights; no margin is added, because r_i bounds every summation order.  Where the device finds the
exact optimum the allowance is 1e-13 |e0|."""
import functools

import numpy as np
import pytest

from oracle import ref_numpy as R
from oracle import synth
from tests import maxflow_reference as F

pytestmark = pytest.mark.gpu


def _block(n, K):
    from phylo_hmrf_amd import Block
    return Block(n, 4, K)


def _expand_and_compare(b, n, edges, w, lp, labels, beta, alpha):
    """set the labels, expand alpha once, compare with kept_side label for label -> the number of labels that changed"""
    p = F.quantised_problem(n, edges, w, lp, labels, beta, alpha)
    # precondition of the reference (top = 0: no active node, or only free-standing ones without a preference)
    assert F.is_power_of_two(p["top"]) or (p["top"] == 0 and not p["cap"].any() and not p["theta"].any()), p["top"]
    want = np.where(F.kept_side(p), alpha, labels)
    b.set_labels(labels)
    changed = b.graph_expansion(beta, alpha)
    got = b.get_labels()
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, ("alpha %d beta %g: %d labels differ from the exact cut, first at node %d: %d for %d (was %d)"
                             % (alpha, beta, wrong.size, wrong[0], got[wrong[0]], want[wrong[0]], labels[wrong[0]]))
    assert changed == int(np.sum(want != labels))
    assert b.graph_expansion(beta, alpha) == 0
    assert np.array_equal(b.get_labels(), want)
    return changed


def _anchored_case(n, edges, w, lp, labels, K, beta, alphas):
    """every alpha on one block of n + 2 nodes: the graph with its anchor pair (whose label follows alpha)"""
    b = None
    total = 0
    try:
        for alpha in alphas:
            na, ea, wa, lpa, laba = F.with_anchor(n, edges, w, lp, labels, beta, alpha)
            if b is None:
                b = _block(na, K)
                b.set_graph(ea, wa)
                b.set_logprob(lpa)
            total += _expand_and_compare(b, na, ea, wa, lpa, laba, beta, alpha)
    finally:
        if b is not None:
            b.close()
    return total


def _plain_case(n, edges, w, lp, labels, K, beta, alphas):
    b = _block(n, K)
    try:
        b.set_graph(edges, w)
        b.set_logprob(lp)
        return sum(_expand_and_compare(b, n, edges, w, lp, labels, beta, alpha) for alpha in alphas)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ B: label for label
@functools.lru_cache(maxsize=None)
def _sparse(n_total, K, seed):
    """n_total nodes WITH the anchor pair: either side of one wave (63, 65) and one workgroup (257), several workgroups (2,049)"""
    rng = np.random.default_rng(7000 + 10 * n_total + seed)
    n = n_total - 2
    beta = (0.5, 1.0, 2.0)[seed % 3]
    return (n,) + F.dyadic_problem(rng, n, F.sparse_pairs(rng, n), K, beta, wmax=2.0) + (beta,)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n_total", [63, 65, 257, 2049])
def test_sparse_random_graphs_label_for_label(n_total, seed):
    n, edges, w, lp, labels, beta = _sparse(n_total, 4, seed)
    assert _anchored_case(n, edges, w, lp, labels, 4, beta, range(4)) > 0          # (some expansion moves something)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sparse_random_graph_of_64_labels(seed):
    n, edges, w, lp, labels, beta = _sparse(257, 64, seed)
    _anchored_case(n, edges, w, lp, labels, 64, beta, (0, 63))


@pytest.mark.parametrize("degree", [64, 61])
def test_a_hub_at_the_degree_limit(degree):
    """node 0 tied to nodes 1 .. degree: D = 64 is the limit of set_graph, 61 is padded to it"""
    n, K, beta = 298, 4, 1.0
    rng = np.random.default_rng(degree)
    pairs = [(i, i + 1) for i in range(n - 1)] + [(0, j) for j in range(2, degree + 1)]
    edges, w, lp, labels = F.dyadic_problem(rng, n, pairs, K, beta, wmax=0.5)
    assert np.bincount(edges.ravel())[0] == degree == np.bincount(edges.ravel()).max()
    assert _anchored_case(n, edges, w, lp, labels, K, beta, range(K)) > 0


@pytest.mark.parametrize("beta", [0.5, 1.0])
@pytest.mark.parametrize("n", [2, 3, 5, 64, 65, 300])
def test_a_far_sink_at_level_n_keeps_every_label(n, beta):
    """A path of n active nodes, all mild sources, whose only sink arc is at the far end: the first node is at residual
    distance n from the sink, the largest level a node can have -- and can reach it, so nothing switches."""
    edges, w, lp, labels = F.far_sink_path(n)
    assert F.quantised_problem(n, edges, w, lp, labels, beta, 1)["top"] == 128.0
    assert _plain_case(n, edges, w, lp, labels, 3, beta, range(3)) == 0          # (alpha = 1 is the case; 0 and 2 are idle)


@pytest.mark.parametrize("depth", [12, 13, 14, 25, 26])
def test_paths_on_either_side_of_the_bfs_windows(depth):
    """the farthest node at BFS level 12 ... 26: the relabelling queues its levels 12 at a time (2-13, 14-25, 26-...)"""
    edges, w, lp, labels = F.far_sink_path(depth)
    assert _anchored_case(depth, edges, w, lp, labels, 3, 1.0, range(3)) == 0
    lp[0, 1] = 48.0                                 # a source the first arc (capacity 32) cannot carry: a prefix switches
    assert _anchored_case(depth, edges, w, lp, labels, 3, 1.0, range(3)) > 0


def test_a_lattice_given_as_a_general_graph():
    """40 x 40, four neighbours, set_graph only (no set_grid): cycles and moderate depth"""
    H = W = 40
    K, beta = 4, 1.0
    rng = np.random.default_rng(40)
    idx = np.arange(H * W).reshape(H, W)
    pairs = list(zip(idx[:, :-1].ravel().tolist(), idx[:, 1:].ravel().tolist())) + \
        list(zip(idx[:-1].ravel().tolist(), idx[1:].ravel().tolist()))
    edges, w, lp, _ = F.dyadic_problem(rng, H * W, pairs, K, beta, wmax=2.0)
    labels = synth.label_image(rng, H, W, K, mean_run=5).reshape(-1)              # regions, so that whole patches switch
    assert _anchored_case(H * W, edges, w, lp, labels, K, beta, range(K)) > 0


def _small(seed, K=4):
    rng = np.random.default_rng(seed)
    n = 20
    return (n,) + F.dyadic_problem(rng, n, F.sparse_pairs(rng, n), K, 1.0, wmax=2.0)


def test_alpha_absent_from_the_labelling():
    n, edges, w, lp, labels = _small(1)
    labels = labels % 3
    _anchored_case(n, edges, w, lp, labels, 4, 1.0, (3,))
    lp[:, 3] += 4.0                                                                # ... and worth taking
    assert _anchored_case(n, edges, w, lp, labels, 4, 1.0, (3,)) > 0


def test_every_node_already_alpha():
    n, edges, w, lp, labels = _small(2)
    labels[:] = 2
    assert F.quantised_problem(n, edges, w, lp, labels, 1.0, 2)["top"] == 0
    assert _plain_case(n, edges, w, lp, labels, 4, 1.0, (2,)) == 0


def test_all_weights_zero():
    """every node decides alone; top is one unary term of 128"""
    n, edges, w, lp, labels = _small(3)
    w[:] = 0.0
    labels[0], lp[0] = 0, (0.0, -128.0, 0.0, 0.0)
    assert _plain_case(n, edges, w, lp, labels, 4, 1.0, (1,)) == int(np.sum((lp[:, 1] > lp[np.arange(n), labels]) & (labels != 1)))


def test_nodes_of_degree_zero():
    """node 20 prefers alpha and has no arc at all (it switches on the "no residual arc" path), node 21 does not"""
    n, edges, w, lp, labels = _small(4)
    lp = np.concatenate([lp, [[-1.0, 0.0, -1.0, -1.0], [0.0, -1.0, -1.0, -1.0]]])
    labels = np.concatenate([labels, [0, 0]])
    b = None
    try:
        na, ea, wa, lpa, laba = F.with_anchor(n + 2, edges, w, lp, labels, 1.0, 1)
        b = _block(na, 4)
        b.set_graph(ea, wa)
        b.set_logprob(lpa)
        _expand_and_compare(b, na, ea, wa, lpa, laba, 1.0, 1)
        got = b.get_labels()
        assert got[n] == 1 and got[n + 1] == 0
    finally:
        if b is not None:
            b.close()


def test_no_edges_at_all():
    n, K = 70, 3
    rng = np.random.default_rng(5)
    lp = -rng.integers(0, 256, (n, K)) / 64.0
    labels = rng.integers(0, K, n)
    labels[0], lp[0] = 0, (0.0, -128.0, 0.0)
    edges, w = np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    assert _plain_case(n, edges, w, lp, labels, K, 2.0, (1,)) > 0


def test_an_exact_tie_keeps_its_labels():
    """theta = (-1, +1) on two nodes tied by a heavy edge: switching both costs exactly 0, so they stay; one input step
    cheaper and both go"""
    edges, w, labels = np.array([[0, 1]]), np.array([8.0]), np.array([0, 0])
    lp = np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    assert _anchored_case(2, edges, w, lp, labels, 3, 1.0, (1,)) == 0
    lp[1, 1] += 1 / 64
    assert _anchored_case(2, edges, w, lp, labels, 3, 1.0, (1,)) == 2


def test_a_flow_that_has_to_travel_2000_hops():
    """A strong source at one end of a path of 2,000 nodes, the only large sink at the other, arcs the source's excess
    saturates: the flow moves about one hop per sweep, far beyond 64 rounds of 24 sweeps, and all but the sink switch."""
    n = 2000
    edges, w, lp, labels = F.deep_path(n)
    assert _plain_case(n, edges, w, lp, labels, 3, 1.0, (1,)) == n - 1


# ------------------------------------------------------------------------------------------------ C: energy
@functools.lru_cache(maxsize=None)
def _knn(seed, n, k, K):
    blk = synth.make_knn_block(seed, n, 4, K, k=k)
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    lp = R.log_multivariate_normal_density_full(blk["X"], blk["means"], blk["covars"])
    return eid, w, lp, np.random.default_rng(seed + 7).integers(0, K, n)


WORST = {}          # the worst (e1 - exact) / allowance seen, printed by every case (recorded in DESIGN.md)


@pytest.mark.parametrize("beta", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("seed,n,k,K,alphas", [(31, 3000, 6, 6, (0, 1, 2, 3, 4, 5)), (32, 2000, 8, 20, (0, 4, 9, 14, 19))])
def test_one_expansion_is_the_exact_optimum_up_to_the_quantisation(seed, n, k, K, alphas, beta):
    eid, w, lp, init = _knn(seed, n, k, K)
    e0 = R.mrf_energy(init, lp, eid, w, beta)[0]
    b = _block(n, K)
    try:
        b.set_graph(eid, w)
        b.set_logprob(lp)
        for alpha in alphas:
            b.set_labels(init)
            changed = b.graph_expansion(beta, alpha)
            lab = b.get_labels()
            got = lab != init
            assert changed == int(got.sum()) and np.all(lab[got] == alpha)
            e1 = R.mrf_energy(lab, lp, eid, w, beta)[0]
            exact, best = F.exact_expansion(n, eid, w, lp, init, beta, alpha)
            allow = F.expansion_allowance(n, eid, w, lp, init, beta, alpha, got, best)
            allow0 = F.expansion_allowance(n, eid, w, lp, init, beta, alpha, got, np.zeros(n, dtype=bool))
            ratio = (e1 - exact) / allow
            WORST["ratio"] = max(WORST.get("ratio", -np.inf), ratio)
            print("\nknn n %d K %d beta %g alpha %d: switched %d (exact %d, %d differ)  e0 %.6f  e1 %.9f  exact %.9f  "
                  "e1 - exact %.3e  allowance %.3e  ratio %.3f (worst so far %.3f)  e1 - e0 %.3e  allowance %.3e"
                  % (n, K, beta, alpha, got.sum(), best.sum(), (got != best).sum(), e0, e1, exact, e1 - exact, allow, ratio,
                     WORST["ratio"], e1 - e0, allow0))
            assert e1 <= exact + allow, (alpha, e1, exact, allow)
            assert e1 <= e0 + allow0, (alpha, e1, e0, allow0)
            assert b.graph_expansion(beta, alpha) == 0
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ E: the solve
def test_converged_on_a_general_graph_means_no_expansion_has_anything_left():
    n, edges, w, lp, labels, beta = _sparse(2049, 4, 0)
    na, ea, wa, lpa, laba = F.with_anchor(n, edges, w, lp, labels, beta, 0)
    b = _block(na, 4)
    try:
        b.set_graph(ea, wa)
        b.set_logprob(lpa)
        b.set_labels(laba)
        res = b.solve(beta, energy_tol_ppb=0)
        assert res["converged"], res
        after = b.get_labels()
        assert R.mrf_energy(after, lpa, ea, wa, beta)[0] < R.mrf_energy(laba, lpa, ea, wa, beta)[0]
        for a in range(4):
            assert b.graph_expansion(beta, a) == 0, a
        assert np.array_equal(b.get_labels(), after)
    finally:
        b.close()
