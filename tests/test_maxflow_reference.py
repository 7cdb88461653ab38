"""CPU: the exact max-flow reference of tests/maxflow_reference.py (used on the GPU by tests/test_gpu_maxflow.py) equals
brute force over all switch sets on graphs of at most 16 active nodes -- the quantised problem label for label (ties by the
"+1 per switched node" rule, then the largest set), the unquantised one in energy -- and the recipe that makes the device's
float32 arithmetic exact leaves no case out."""
import numpy as np
import pytest

from oracle import ref_numpy as R
from tests import maxflow_reference as F


def _random_problem(seed, dyadic):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 17))
    pairs = F.sparse_pairs(rng, n) if seed % 2 else [(i, i + 1) for i in range(n - 1)]
    K = 3
    edges, w, lp, labels = F.dyadic_problem(rng, n, pairs, K, 1.0)
    if not dyadic:
        w = rng.random(len(edges)) * 1.5 + 0.05
        lp = -rng.random((n, K)) * 3.0
    return n, edges, w, lp, labels, float(rng.choice([0.5, 1.0, 2.0])) if dyadic else 0.9


@pytest.mark.parametrize("dyadic", [True, False])
def test_reference_equals_brute_force_on_small_graphs(dyadic):
    switched_any = 0
    for seed in range(40):
        n, edges, w, lp, labels, beta = _random_problem(seed, dyadic)
        for alpha in (1, 2):
            want_set, want_e = F.brute_force(n, edges, w, lp, labels, beta, alpha)
            got_set = F.kept_side(F.quantised_problem(n, edges, w, lp, labels, beta, alpha))
            assert np.array_equal(got_set, want_set), (seed, alpha, got_set, want_set)
            e, sw = F.exact_expansion(n, edges, w, lp, labels, beta, alpha)
            assert abs(e - want_e) <= 1e-9, (seed, alpha, e, want_e)
            cand = np.where(sw, alpha, labels)
            assert e == R.mrf_energy(cand, lp, edges, w, beta)[0]
            switched_any += int(want_set.any())
    assert switched_any >= 20                     # (the cases are not all "nothing switches")


def test_dyadic_ties_go_by_the_quantum_then_by_the_largest_set():
    """Two nodes of label 0, one edge of weight 1: switching both costs theta_0 + theta_1.  At exactly 0 the "+1" per
    switched node keeps the labels; one input step below 0 both switch; a node whose quantised cost is exactly 0 (ceil = -1)
    joins the switched set (the largest set among the minima)."""
    edges, w, labels = np.array([[0, 1]]), np.array([1.0]), np.array([0, 0])
    for d, want in ((0.0, [False, False]), (-1 / 64, [True, True])):
        lp = np.array([[0.0, 1.0, 0], [0.0, -1.0 - d, 0]])          # theta = (-1, 1 + d)
        p = F.quantised_problem(2, edges, w, lp, labels, 1.0, 1)
        assert F.kept_side(p).tolist() == want == F.brute_force(2, edges, w, lp, labels, 1.0, 1)[0].tolist()
    lp = np.array([[0.0, 2.0 ** -25, 0], [0.0, -1.0, 0]])          # node 0: scale * theta = -1/2, ceil + 1 = 1: kept
    assert F.quantised_problem(2, edges, w, lp, labels, 1.0, 1)["cost"][0] == 1
    lp = np.array([[0.0, 2.0 ** -24, 0], [0.0, -1.0, 0]])          # scale * theta = -1: cost 0, no arc to source or sink
    p = F.quantised_problem(2, edges[:0], w[:0], lp, labels, 1.0, 1)
    assert p["cost"][0] == 0 and F.kept_side(p).tolist() == [True, False]
    assert F.brute_force(2, edges[:0], w[:0], lp, labels, 1.0, 1)[0].tolist() == [True, False]


@pytest.mark.parametrize("n", [2, 3, 5, 64, 65, 300])
@pytest.mark.parametrize("beta", [0.5, 1.0, 2.0])
def test_a_path_whose_only_sink_is_at_the_far_end_switches_nothing(n, beta):
    edges, w, lp, labels = F.far_sink_path(n)
    p = F.quantised_problem(n, edges, w, lp, labels, beta, 1)
    assert p["top"] == 128.0 and int((p["cost"] > 0).sum()) == 1 and p["cost"][n - 1] == 2 ** 24 + 1
    assert not F.kept_side(p).any()
    e, sw = F.exact_expansion(n, edges, w, lp, labels, beta, 1)
    assert not sw.any() and e == R.mrf_energy(labels, lp, edges, w, beta)[0]
    if n <= 5:
        assert not F.brute_force(n, edges, w, lp, labels, beta, 1)[0].any()


def test_the_deep_path_switches_all_but_its_sink():
    for n in (12, 2000):
        edges, w, lp, labels = F.deep_path(n)
        p = F.quantised_problem(n, edges, w, lp, labels, 1.0, 1)
        assert F.is_power_of_two(p["top"])
        got = F.kept_side(p)
        assert got[:n - 1].all() and not got[n - 1]
        if n == 12:
            assert np.array_equal(got, F.brute_force(n, edges, w, lp, labels, 1.0, 1)[0])


def test_the_anchor_makes_top_a_power_of_two_on_every_random_problem():
    """1,200 problems of 2-31 nodes, path and sparse, K = 3, alpha in {1, 2}: none is left out."""
    for seed in range(300):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(2, 32))
        pairs = F.sparse_pairs(rng, n) if seed % 2 else [(i, i + 1) for i in range(n - 1)]
        beta = (0.5, 1.0, 2.0)[seed % 3]
        edges, w, lp, labels = F.dyadic_problem(rng, n, pairs, 3, beta)
        for alpha in (1, 2):
            for lab in (labels, np.where(labels == alpha, 0, labels)):
                p = F.quantised_problem(*F.with_anchor(n, edges, w, lp, lab, beta, alpha), beta, alpha)
                assert p["top"] == 128.0 and F.is_power_of_two(p["top"])
                # exact in float32: every capacity and cost is an integer before it is rounded
                assert np.all(p["scale"] * p["theta"] == np.round(p["scale"] * p["theta"]))


def test_allowance_covers_the_quantised_optimum_and_is_far_below_the_old_one():
    """The set the quantised problem picks (what a correct device expansion returns on real-valued inputs, up to float32
    rounding that the allowance counts as well) is within the allowance of the true optimum and of the energy before; the
    allowance counts the nodes and arcs in which the two sets differ, far below n * (2 max|lp| + sum w) / 2^24."""
    worst = 0.0
    for seed in range(40):
        n, edges, w, lp, labels, beta = _random_problem(seed, False)
        e0 = R.mrf_energy(labels, lp, edges, w, beta)[0]
        for alpha in (1, 2):
            got = F.kept_side(F.quantised_problem(n, edges, w, lp, labels, beta, alpha))
            e1 = R.mrf_energy(np.where(got, alpha, labels), lp, edges, w, beta)[0]
            e, best = F.exact_expansion(n, edges, w, lp, labels, beta, alpha)
            allow = F.expansion_allowance(n, edges, w, lp, labels, beta, alpha, got, best)
            assert e1 <= e + allow and e1 <= e0 + F.expansion_allowance(n, edges, w, lp, labels, beta, alpha, got, got & False)
            old = n * max(2 * np.abs(lp).max() + w.sum(), 1.0) / 2 ** 24
            assert allow < 0.25 * old
            if allow > 0:
                worst = max(worst, (e1 - e) / allow)
    assert worst <= 1.0
