"""GPU: posterior_kernel<S, VEC, WRITE_POST, GRID> (phmrf_posterior_stats, phmrf_posterior_stats_dev) in every compiled
form against the shift-invariant float64 reference of tests/posterior_reference.py.

What runs here, per template axis and launcher decision (csrc/kernels.hip: launch_posterior_s):
  S            1 .. 8, each with every adjacency form below
  VEC          1 (K odd), 2 (K % 4 == 2), 4 (K % 4 == 0); K in {1, 2, 3, 5, 6, 7, 16, 17, 20, 33, 40, 56, 64}
  WRITE_POST   both, in every case (the statistics-only call must return what the call with posteriors returns)
  GRID         true  : set_graph + set_grid(H, W, diag, 8), diagonal and rectangular blocks
               false : explicit rows, D == 8 (complete stencil; random graph with ragged rows and isolated nodes);
                       the j += 4 loop with D == 4 (ragged, node 0 isolated) and D == 12 (three trips, full rows)
  reduction    f64 atomics (default) and PHMRF_DETERMINISTIC=1 (one wave per workgroup + posterior_reduce_kernel)
  tile rows    256 and 128 from the launcher's LDS rule (K >= 40 at S = 8 down to K >= 60 at S = 1 run 128 rows),
               64 in deterministic mode; n on both sides of each edge; both grid-stride wraps (deterministic: more than
               2048 * 64 nodes, default: more than cap * 256 nodes)

Tolerances are the project's (tests/test_gpu_estep.py): posteriors 2e-5 absolute; statistics rtol 2e-5 with
atol 1e-6 * max|ref|; cost scalars rtol 1e-5.  Cost [1] (and [3], which contains it) gets an absolute term as well,
derived in tests/posterior_cases.py (_cost1_atol), for the nodes whose term -log(ppn + 1e-16) is below what f32 resolves.
The reference reads the inputs as the device holds them: logprob, observations and weights rounded to f32.

What the file notices: each of these changes to posterior_kernel, built and run once against it, fails the tests named
(F = test_form_matrix_against_reference, D = test_deterministic_mode_against_reference, W = the two second-tile tests,
E = test_estimate_types, L = test_real_magnitude_exact_lattice, C = test_real_magnitude_after_the_emission_kernel,
V = test_posterior_stats_dev_is_the_host_call, B = test_large_beta_..., U = test_summary_kernel_...; cases failed / run):
  no mirrored write in the flush and in posterior_reduce_kernel   F 51/57, D 9/10, W 2/2, E 4/4, L 6/6, V 4/4, B 2/2
  use_w forced to 1                                               F 26, D 3, E 4/4, B 2/2, C 2/4, U 3/4
  no isolated-node branch in phase 1                              F 21, D 4, E 2, V 2, U 4/4
  r <= rows in phase 4                                            F 44, D 6, W 2/2, L 6/6, V 4/4, B 2/2, C 1
  no max shift in phase 3 (m = 0)                                 L 6/6, C 4/4, U 2
  fb from ps + r instead of ps + r + 1                            F 57/57, D 10/10, W 2/2, E 4/4, L 6/6, V 4/4, B 2/2
"""
import numpy as np
import pytest

from oracle import ref_numpy as R
from tests import posterior_reference as P
from tests.posterior_cases import (KEYS, _block, _f32, default_wrap_nodes, _observations, _labels, _cost1_atol,
                                   _assert_costs, _assert_stats, _Case, _case, FORM_CASES)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("S,K,form,n,beta,et,mode", FORM_CASES)
def test_form_matrix_against_reference(S, K, form, n, beta, et, mode):
    c = _case(S, K, form, n, beta, et, mode)
    if form == "isolated":
        assert np.count_nonzero(c.deg == 0) >= 0.1 * n
    if form == "deg12":
        assert c.D == 12 and np.count_nonzero(c.deg == 12) > 0
    if form == "ragged4":
        assert c.deg[0] == 0
    b = c.block()
    stats, costs, post = c.check(b)
    if beta == 0.0:                                    # no pair term: softmax(logprob), and ppn = 1 / K for every node
        assert np.max(np.abs(post - P.softmax_rows(c.lp))) < 2e-5
        np.testing.assert_allclose(costs[1], -n * np.log(1.0 / K + 1e-16), rtol=1e-5, atol=c.atol1)    # (atol1 == 0 unless K == 1)
        assert (c.atol1 == 0.0) == (K > 1)
        assert costs[0] == 0.0
    if mode == "absent" and K > 1:
        assert not np.any(c.labels == K - 1) and c.stats["post"][K - 1] > 0.0
    b.close()


@pytest.mark.parametrize("form,S,K", [("grid_rect", 3, 6), ("explicit8", 5, 7), ("deg12", 2, 20), ("isolated", 7, 3)])
def test_estimate_types(form, S, K, monkeypatch):
    """1 and 2 are 0 (weights of one) bit for bit; 3 reads the weights and differs where they are not all one -- in the
    default build and with the ordered reduction, where the statistics and costs are bit for bit the same as well"""
    for det in (False, True):
        if det:
            monkeypatch.setenv("PHMRF_DETERMINISTIC", "1")
        else:
            monkeypatch.delenv("PHMRF_DETERMINISTIC", raising=False)
        c = _case(S, K, form, 320, 1.3, 0, "random")
        assert np.any(c.w < 0.9)
        b = c.block()
        out = {et: b.posterior_stats(1.3, et, want_posteriors=True) for et in (0, 1, 2, 3)}
        for et in (1, 2):
            assert np.array_equal(out[et][2], out[0][2])
            if det:
                assert all(np.array_equal(out[et][0][key], out[0][0][key]) for key in KEYS) and np.array_equal(out[et][1], out[0][1])
            else:
                np.testing.assert_allclose(out[et][1], out[0][1], rtol=1e-9)
        post3, costs3, stats3 = P.posteriors_costs_stats(c.labels, c.lp, c.X, c.eid, c.w, 1.3, 3)
        assert np.max(np.abs(post3 - c.post)) > 1e-2                    # (the reference itself tells the two apart)
        assert np.max(np.abs(out[3][2] - out[0][2])) > 1e-2
        assert np.max(np.abs(out[3][2] - post3)) < 2e-5
        _assert_stats(out[3][0], stats3, c.n)
        _assert_costs(out[3][1], costs3, _cost1_atol(c.labels, c.eid, c.w, K, 1.3, 3))
        assert costs3[0] < 0.95 * c.costs[0] and out[3][1][0] < 0.95 * out[0][1][0]    # sum of w' [l != l'], w < 1 against w' = 1
        b.close()


@pytest.mark.parametrize("form", ["grid_rect", "explicit8"])
def test_large_beta_the_epsilon_inside_the_log_decides(form):
    """beta = 6, estimate_type 0: a node that disagrees with all eight neighbours has ppn = e^-48 / (1 + ...) ~ 1e-21, far
    below the 1e-16 inside the log, so its term of cost [1] is -log(1e-16 + 1e-21) = 36.84 and not 48"""
    S, K = 4, 5
    c = _case(S, K, form, 360, 6.0, 0, "one")
    H, W = c.geom[0], c.geom[1]
    ii, jj = np.divmod(np.arange(H * W), W)
    lone = (ii % 3 == 1) & (jj % 3 == 1)
    c = c.relabelled(np.where(lone, 1, 0))
    V = R.potts_matrix(K, 6.0)
    ppn = P.softmax_rows(-R.pairwise_compare(c.labels, c.eid, c.w, V, 0))[np.arange(c.n), c.labels]
    assert np.count_nonzero(lone) == 40 and np.all(ppn[lone] < 1e-18)
    assert c.costs[1] > 40 * 36.8 and c.costs[1] < 40 * 36.9 + (c.n - 40) * 1.0
    b = c.block()
    c.check(b)
    b.close()


# ---- (b) real magnitude ----------------------------------------------------------------------------------------------
def _exact_case(S, form, diag):
    """logprob on the 1/16 lattice in [-2^15, 0], weights on the 1/8 lattice, beta = 1.25: every logprob + beta * h is
    a multiple of 1/32 below 2^15 in size -- 20 bits -- and so are the differences to the row maximum: the device's
    soft-max reads the very numbers the reference reads, at the magnitude of a fit"""
    K, beta = 7, 1.25
    N, H, W = 45, 36, 50
    geom = (N, N, True) if diag else (H, W, False)
    n = N * (N + 1) // 2 if diag else H * W
    rng = np.random.default_rng(77 + S + 10 * diag)
    X = _observations(rng, n, S)
    eid = np.int64(R.grid_edges(X, geom[0], geom[1], diag, 8)[:, 0:2])
    w = rng.integers(1, 9, len(eid)) / 8.0
    top = -rng.integers(0, (2 ** 15 - 700) * 16, n) / 16.0
    gap = rng.integers(0, 500 * 16, (n, K)) / 16.0
    gap[:, 0] = 0.0
    planted = [0.0, 1.0 / 16, 1.0, 200.0 + 1.0 / 16, 613.0]              # gap of the second state to the first
    for r, g in enumerate(planted * 8):
        gap[r, 1:] = np.maximum(gap[r, 1:], g + 1.0 / 8)
        gap[r, 1] = g
    gap[40:48, 1:] = 100.0 + rng.integers(1, 400 * 16, (8, K - 1)) / 16.0   # every state but one more than 100 below the maximum
    lp = top[:, None] - gap
    for r in range(n):                                                  # the maximum is not always state 0
        lp[r] = np.roll(lp[r], r % K)
    assert lp.min() >= -2.0 ** 15 and lp.max() <= 0.0 and np.array_equal(lp * 16, np.round(lp * 16))
    labels = _labels(rng, "argmax", lp)
    h = np.zeros((n, K))
    np.add.at(h, (eid[:, 0], labels[eid[:, 1]]), w)
    np.add.at(h, (eid[:, 1], labels[eid[:, 0]]), w)
    a = lp + beta * h
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)   # exactly representable: one fma, no rounding
    assert np.array_equal(lp.astype(np.float32).astype(np.float64), lp)
    return _Case(S, K, form, beta, 3, X, eid, w, geom, lp, labels)


def _check_summary(c, b, post_dev):
    """posterior_summary_kernel has no S template and its own tile height: conf is the statistics kernel's posterior of
    the node's label, the entropy finite and >= 0"""
    conf, top, ent = b.posterior_summary(c.beta, c.et, want_entropy=True)
    assert np.max(np.abs(conf.astype(np.float64) - post_dev[np.arange(c.n), c.labels])) <= 1e-7
    assert np.all(np.isfinite(ent)) and np.all(ent >= 0.0)
    assert np.max(np.abs(conf - c.post[np.arange(c.n), c.labels])) < 2e-5


@pytest.mark.parametrize("S,form,diag", [(3, "grid", True), (4, "explicit8", False), (8, "grid", False), (3, "explicit8", True),
                                         (4, "grid", True), (8, "explicit8", True)])
def test_real_magnitude_exact_lattice(S, form, diag):
    c = _exact_case(S, form, diag)
    srt = np.sort(c.lp, axis=1)
    d = srt[:, -1] - srt[:, -2]
    assert {0.0, 1.0 / 16, 1.0} <= set(d[:40]) and d.max() > 200 and np.abs(c.lp).max() > 3e4
    assert np.any(srt[:, -1] - srt[:, -2] > 100)
    b = c.block()
    stats, costs, post = c.check(b)
    assert np.all(np.isfinite(post))
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-5)
    _check_summary(c, b, post)
    b.close()


@pytest.mark.parametrize("S,K,et", [(2, 5, 0), (5, 3, 3), (6, 7, 0), (7, 9, 3)])
def test_real_magnitude_after_the_emission_kernel(S, K, et):
    """emission -> posterior_stats on the resident logprob, with a near-singular covariance (only the 2e-3 jitter in one
    direction) and observations scaled out until |logprob| passes 1e3.  The reference reads the device's own logprob.

    Bound per row.  The device forms a_k = fma(beta, h_k, lp_k) in f32: |da_k| <= 2^-24 |a_k|.  For p = softmax(a),
    dp_k = p_k (da_k - sum_j p_j da_j), so |dp_k| <= 2 p_k max_j |da_j| <= 2^-23 max_j |a_j|.  On top of the project's
    2e-5 (exp, sum, reciprocal): |post - ref| <= 2e-5 + 2^-23 * max_k |lp_ik + beta h_ik| in row i."""
    rng = np.random.default_rng(S * 100 + K)
    n, beta = 1500, 0.7
    H, W = 30, 50
    A = rng.standard_normal((K, S, S))
    A[:, :, -1] = 0.0                                   # rank S - 1: the jitter alone holds the last direction
    cov = np.einsum("kij,klj->kil", A, A) * 0.3 + 2e-3 * np.eye(S)
    mu = rng.uniform(0, 4, (K, S))
    X = _f32(np.abs(mu[rng.integers(0, K, n)] + 1.5 * 0.7 * rng.standard_normal((n, S))))
    e = R.grid_edges(X, H, W, False, 8)
    w, eid = R.edge_weights_from_distance(e, 0.5)
    w = _f32(w)
    b = _block(n, S, K)
    b.set_observations(X)
    b.set_graph(eid, w)
    b.set_grid(H, W, False, 8)
    b.emission(mu, cov)
    lp = b.get_logprob()
    assert np.all(np.isfinite(lp)) and np.abs(lp).max() > 1e3, np.abs(lp).max()
    assert np.median(np.abs(lp).max(axis=1)) > 1e2
    labels = np.where(rng.random(n) < 0.8, np.argmax(lp, 1), rng.integers(0, K, n))
    b.set_labels(labels)
    stats, costs, post = b.posterior_stats(beta, et, want_posteriors=True)
    post_ref, costs_ref, _ = P.posteriors_costs_stats(labels, lp, X, eid, w, beta, et)
    h = np.zeros((n, K))
    ww = w if et == 3 else np.ones_like(w)
    np.add.at(h, (eid[:, 0], labels[eid[:, 1]]), ww)
    np.add.at(h, (eid[:, 1], labels[eid[:, 0]]), ww)
    bound = 2e-5 + 2.0 ** -23 * np.max(np.abs(lp + beta * h), axis=1)
    err = np.max(np.abs(post - post_ref), axis=1)
    print("max |lp| %.3g, worst row: err %.2e of bound %.2e" % (np.abs(lp).max(), err.max(), bound[np.argmax(err / bound)]))
    assert np.all(err <= bound)
    np.testing.assert_allclose(costs[2], costs_ref[2], rtol=1e-5)
    np.testing.assert_allclose(costs[0], costs_ref[0], rtol=1e-5)
    np.testing.assert_allclose(stats["post"].sum(), n, rtol=1e-6)
    b.close()


# ---- (c) the ordered reduction against the reference -----------------------------------------------------------------
DET_CASES = [(1, 17, "grid_rect", 63, 1.3, 3, "argmax"), (2, 3, "explicit8", 64, 0.3, 0, "random"), (3, 64, "ragged4", 65, 1.3, 3, "absent"),
             (4, 20, "deg12", 127, 6.0, 3, "random"), (5, 7, "isolated", 128, 1.3, 1, "argmax"), (6, 2, "grid_diag", 136, 0.0, 2, "random"),
             (7, 33, "grid_rect", 129, 1.3, 3, "one"), (8, 16, "explicit8", 192, 0.3, 3, "argmax"), (8, 64, "deg12", 193, 1.3, 0, "random"),
             (5, 1, "ragged4", 64, 1.3, 3, "random")]


@pytest.mark.parametrize("S,K,form,n,beta,et,mode", DET_CASES)
def test_deterministic_mode_against_reference(S, K, form, n, beta, et, mode, monkeypatch):
    """PHMRF_DETERMINISTIC=1 (read when the block is created): 64-row workgroups of one wave, per-workgroup rows added in
    workgroup order -- the same numbers as the reference, and the same bits call after call and block after block"""
    monkeypatch.setenv("PHMRF_DETERMINISTIC", "1")
    c = _case(S, K, form, n, beta, et, mode)
    b = c.block()
    s1, c1, p1 = c.check(b, deterministic=True)
    s2, c2, p2 = b.posterior_stats(beta, et, want_posteriors=True)
    b.close()
    b = c.block()
    s3, c3, p3 = b.posterior_stats(beta, et, want_posteriors=True)
    b.close()
    for s, cc, p in ((s2, c2, p2), (s3, c3, p3)):
        assert all(np.array_equal(s[key], s1[key]) for key in KEYS) and np.array_equal(cc, c1) and np.array_equal(p, p1)


def _wrap_case(N, S, K):
    """an N x N diagonal block with more nodes than one pass of the kernel's grid covers"""
    n = N * (N + 1) // 2
    rng = np.random.default_rng(N + K)
    X = _observations(rng, n, S)
    w, eid = R.edge_weights_from_distance(R.grid_edges(X, N, N, True, 8), 0.5)
    lp = _f32(rng.normal(0.0, 3.0, (n, K)) - 5.0)
    return _Case(S, K, "grid_diag", 1.3, 3, X, eid, _f32(w), (N, N, True), lp, _labels(rng, "argmax", lp))


def test_deterministic_mode_second_tile_per_workgroup(monkeypatch):
    """more than 2048 * 64 = 131,072 nodes: the grid is capped and every workgroup strides to a second tile"""
    monkeypatch.setenv("PHMRF_DETERMINISTIC", "1")
    c = _wrap_case(529, 2, 3)
    assert c.n == 140185 > 2048 * 64
    b = c.block()
    c.check(b, deterministic=True)
    b.close()


# ---- (d) the default path's second tile ------------------------------------------------------------------------------
def test_default_path_second_tile_per_workgroup():
    """K = 3, S = 2 is the smallest LDS class: 1280 workgroups of 256 rows; above 327,680 nodes the first workgroups wrap"""
    c = _wrap_case(825, 2, 3)
    assert c.n == 340725 > default_wrap_nodes(3, 2)
    b = c.block()
    c.check(b)
    b.close()


# ---- (e) results left on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("S,K,form,n", [(3, 7, "grid_rect", 513), (8, 20, "deg12", 257)])
def test_posterior_stats_dev_is_the_host_call(S, K, form, n, det, monkeypatch):
    import torch
    from phylo_hmrf_amd.block import pack_stats
    if det:
        monkeypatch.setenv("PHMRF_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("PHMRF_DETERMINISTIC", raising=False)
    c = _case(S, K, form, n, 1.3, 3, "argmax")
    b = c.block()
    stats, costs, _ = b.posterior_stats(c.beta, c.et)
    _assert_stats(stats, c.stats, n)
    ns = b.n_stats()
    host = np.concatenate([pack_stats(stats), costs])
    out = torch.full((ns + 4,), 1e30, dtype=torch.float64, device="cuda")
    for call in range(2):                               # the second call overwrites: nothing accumulates in the buffer
        b.posterior_stats_dev(c.beta, c.et, out.data_ptr())
        b.sync()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        if det:
            assert np.array_equal(got, host), call
        else:
            np.testing.assert_allclose(got, host, rtol=1e-9, err_msg=str(call))
    b.close()


# ---- (f) the summary kernel at the new shapes ------------------------------------------------------------------------
@pytest.mark.parametrize("S,K,form,n,beta,et", [(2, 20, "deg12", 320, 1.3, 0), (7, 3, "isolated", 320, 1.3, 0), (3, 64, "deg12", 257, 6.0, 3),
                                                (7, 40, "isolated", 257, 1.3, 2)])
def test_summary_kernel_on_wide_rows_and_isolated_nodes(S, K, form, n, beta, et):
    c = _case(S, K, form, n, beta, et, {0: "random", 3: "absent", 2: "argmax"}[et])
    b = c.block()
    _, _, post = b.posterior_stats(beta, et, want_posteriors=True)
    assert np.max(np.abs(post - c.post)) < 2e-5
    _check_summary(c, b, post)
    b.close()
