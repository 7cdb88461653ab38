"""CPU: tests/posterior_reference.py (the shift-invariant float64 yardstick of posterior_kernel) against the oracle's
restatement of the reference formula where that formula is finite, against the C restatement on the recorded fixtures,
and at the log-likelihood magnitudes where the un-shifted formula is not finite -- the reason it exists."""
import os

import numpy as np
import pytest

from oracle import estep_c, ref_numpy as R
from oracle import synth
from tests import posterior_reference as P
from tests import posterior_cases as GP

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _block(seed=4, N=60, K=7, S=4):
    blk = synth.make_block(seed, N, N, S, K, True)
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    return blk["X"], eid, w


@pytest.mark.parametrize("et", [0, 3])
@pytest.mark.parametrize("beta", [0.0, 1.3])
def test_equals_the_oracle_where_the_unshifted_formula_is_finite(et, beta):
    X, eid, w = _block()
    n, K = X.shape[0], 7
    rng = np.random.default_rng(11)
    lp = rng.normal(-20.0, 8.0, (n, K))
    labels = rng.integers(0, K, n)
    labels[rng.random(n) < 0.5] = 3                 # agreeing neighbourhoods as well as mixed ones
    post_ref, pc, pcn, uc, c1 = R.compute_posteriors_graph(labels, lp, eid, w, R.potts_matrix(K, beta), et)
    assert np.all(np.isfinite(post_ref))
    post, costs, stats = P.posteriors_costs_stats(labels, lp, X, eid, w, beta, et)
    assert np.max(np.abs(post - post_ref)) <= 1e-12
    np.testing.assert_allclose(costs / n, [pc, pcn, uc, c1], rtol=1e-12)
    st_ref = R.sufficient_statistics(post_ref, X)
    for key in ("post", "obs", "obs*obs.T"):
        np.testing.assert_allclose(stats[key], st_ref[key], rtol=1e-12)


def test_isolated_nodes_follow_the_oracle():
    """no edges at all (every node isolated: pp = V[l_i, :]) and a graph in which only some nodes are"""
    rng = np.random.default_rng(2)
    n, K = 50, 4
    lp, labels, X = rng.normal(-3.0, 2.0, (n, K)), rng.integers(0, K, n), rng.random((n, 2))
    for eid in (np.zeros((0, 2), dtype=np.int64), np.stack([np.arange(0, 20), np.arange(1, 21)], 1)):
        w = rng.uniform(0.2, 1.0, len(eid))
        post_ref, pc, pcn, uc, c1 = R.compute_posteriors_graph(labels, lp, eid, w, R.potts_matrix(K, 0.8), 3)
        post, costs, _ = P.posteriors_costs_stats(labels, lp, X, eid, w, 0.8, 3)
        assert np.max(np.abs(post - post_ref)) <= 1e-12
        np.testing.assert_allclose(costs / n, [pc, pcn, uc, c1], rtol=1e-12)


@pytest.mark.parametrize("et", [0, 3])
def test_equals_the_c_restatement_on_the_recorded_fixtures(et):
    g = np.load(os.path.join(G, "posteriors_et%d.npz" % et))
    X, lp, labels, w, beta = g["X"], g["logprob"], g["labels"], g["w"], float(g["beta"])
    n, K = lp.shape
    S = X.shape[1]
    eid = np.int64(g["edges"][:, 0:2])
    stats_c, costs_c, post_c = estep_c.posterior_stats(X, lp, eid, w, labels, beta, et)
    post, costs, stats = P.posteriors_costs_stats(labels, lp, X, eid, w, beta, et)
    np.testing.assert_allclose(post, post_c, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(post, g["posteriors"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(stats["post"], stats_c[:K], rtol=1e-12)
    np.testing.assert_allclose(stats["obs"], stats_c[K:K + K * S].reshape(K, S), rtol=1e-12)
    np.testing.assert_allclose(stats["obs*obs.T"], stats_c[K + K * S:].reshape(K, S, S), rtol=1e-12)
    # (the C restatement returns the reference's per-node means, this one the un-normalised sums of include/phmrf.h)
    np.testing.assert_allclose(costs / n, costs_c, rtol=1e-12)


def test_stays_finite_at_the_magnitude_of_a_fit_where_the_unshifted_formula_does_not():
    X, eid, w = _block(seed=6, N=62)
    n, K = X.shape[0], 7
    rng = np.random.default_rng(3)
    lp = -rng.uniform(0.0, 2e4, (n, K))
    labels = rng.integers(0, K, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        post_ref = R.compute_posteriors_graph(labels, lp, eid, w, R.potts_matrix(K, 1.0), 3)[0]
    bad = ~np.all(np.isfinite(post_ref), axis=1)
    assert bad.sum() > n // 2, bad.sum()                        # 0 / 0: every exp of the row underflowed
    post, costs, stats = P.posteriors_costs_stats(labels, lp, X, eid, w, 1.0, 3)
    assert np.all(np.isfinite(post)) and np.all(post >= 0.0)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.all(np.isfinite(costs))
    assert all(np.all(np.isfinite(v)) for v in stats.values())
    np.testing.assert_allclose(stats["post"].sum(), n, rtol=1e-12)
    # and on the rows the un-shifted formula does survive, the two agree
    ok = ~bad
    assert ok.any()
    assert np.max(np.abs(post[ok] - post_ref[ok])) <= 1e-12


def test_a_constant_added_to_a_row_of_logprob_changes_no_posterior():
    X, eid, w = _block(seed=8, N=40, K=5)
    n, K = X.shape[0], 5
    rng = np.random.default_rng(9)
    lp = rng.normal(-30.0, 10.0, (n, K))
    labels = rng.integers(0, K, n)
    c = rng.uniform(-5e3, 5e3, (n, 1))
    p0, c0, s0 = P.posteriors_costs_stats(labels, lp, X, eid, w, 1.3, 3)
    p1, c1, s1 = P.posteriors_costs_stats(labels, lp + c, X, eid, w, 1.3, 3)
    # lp + c rounds each entry at 2^-53 * 5e3: 6e-13 in the exponent
    assert np.max(np.abs(p1 - p0)) <= 1e-11
    for key in s0:
        np.testing.assert_allclose(s1[key], s0[key], rtol=1e-10)
    np.testing.assert_allclose(c1[:2], c0[:2], rtol=1e-12)          # the pair terms do not read logprob
    np.testing.assert_allclose(c1[2], c0[2] - c.sum(), rtol=1e-10)  # the unary cost moves by the constants


# ---- the shapes and the bounds of tests/test_gpu_posterior.py (its own tests need a GPU; these do not) ---------------
def test_tile_rule_covers_both_default_heights():
    """(the shapes of tests/test_gpu_posterior.py are what the launcher's rule says they are -- 64 rows exist in deterministic mode only)"""
    assert GP.tile_rows(20, 4) == (256, 29024) and GP.tile_rows(33, 8)[0] == 256
    assert GP.tile_rows(64, 1)[0] == 128 and GP.tile_rows(64, 8) == (128, 60928) and GP.tile_rows(56, 8) == (128, 53952)
    assert all(GP.tile_rows(K, S)[0] >= 128 for K in range(1, 65) for S in range(1, 9))
    assert GP.default_wrap_nodes(40, 4) == 196608 and GP.default_wrap_nodes(3, 2) == 327680


def test_tile_rule_is_the_launchers():
    """tile_rows and default_wrap_nodes restate launch_posterior_s; the lines they restate are pinned in its source, so a
    change of the launcher's rule fails here until the restatement follows"""
    csrc = os.path.join(os.path.dirname(G), os.pardir, "phylo_hmrf_amd", "csrc")
    kernels = " ".join(open(os.path.join(csrc, "kernels.hip")).read().split())
    common = " ".join(open(os.path.join(csrc, "common.h")).read().split())
    assert "while (TB > 64 && (size_t)TB * (Kp + Mp) * sizeof(float) + acc_bytes > 64 * 1024 - 256) TB >>= 1;" in kernels
    assert ("(lds <= 32 * 1024 ? 256 * 5 : (lds <= 40 * 1024 ? 256 * 4 : (lds <= 53 * 1024 ? 256 * 3 : 256 * 8))) * (256 / TB)"
            in kernels)
    assert "constexpr int Mp = ((S + 1) % 2 == 0) ? S + 2 : S + 1;" in kernels
    assert "constexpr int POST_PARTIAL_ROWS = 2048;" in common and "constexpr int POST_DET_TB = 64;" in common


def test_form_matrix_covers_what_it_claims():
    """tests/test_gpu_posterior.py: every S with every adjacency form; every K class, beta, estimate_type, labelling, tile height and edge"""
    assert {(c[0], c[2]) for c in GP.FORM_CASES} >= {(S, form) for S in range(1, 9) for form in GP.FORMS}
    Ks = {c[1] for c in GP.FORM_CASES}
    assert Ks >= set(GP.K_CYCLE) | {56} and {K % 4 for K in Ks} >= {0, 1, 2, 3} and {min(K % 16, 2) for K in Ks} == {0, 1, 2}
    assert {c[4] for c in GP.FORM_CASES} == set(GP.BETAS) and {c[5] for c in GP.FORM_CASES} == {0, 1, 2, 3} and {c[6] for c in GP.FORM_CASES} == set(GP.MODES)
    edges = {(GP.tile_rows(c[1], c[0])[0], c[3] - GP.tile_rows(c[1], c[0])[0]) for c in GP.FORM_CASES}
    assert edges >= {(TB, d) for TB in (128, 256) for d in (-1, 0, 1)} and any(d == TB + 1 for TB, d in edges)
    ns = {c[3] for c in GP.FORM_CASES}
    assert ns >= {1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 3080}
    assert 40 <= len(GP.FORM_CASES) <= 60 and len(set(GP.FORM_CASES)) == len(GP.FORM_CASES)


def test_gpu_cases_count_the_stencil_and_bound_only_the_unresolvable_terms():
    assert GP._stencil_entries(3, 3, False) == 4 * 3 + 4 * 5 + 8 and GP._stencil_entries(3, 3, True) == 2 * 10
    c = GP._case(3, 6, "grid_rect", 320, 1.3, 0, "random")
    assert 2 * len(c.eid) == GP._stencil_entries(*c.geom)
    one = c.relabelled(np.zeros(c.n, dtype=np.int64))
    # all neighbours agree: t = log(1 + y), y <= (K - 1) e^(-beta Wtot); the nodes with t < (2 + K / 2) * 2^-23 / rtol = 0.06
    # get their f32 bound; beta = 0: ppn = 1 / K, every term is log K and rtol alone holds
    assert 0.0 < one.atol1 < c.n * (2.0 + 3.0 + np.expm1(0.06) * (2.0 + 5.0 * 1.3 * 8)) * 2.0 ** -23
    assert GP._cost1_atol(c.labels, c.eid, c.w, 6, 0.0, 0) == 0.0
    assert GP._cost1_atol(c.labels, c.eid, c.w, 6, 1.3, 0) < 0.1 * one.atol1
