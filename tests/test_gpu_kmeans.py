"""The initialisation's device code on the GPU: kmeans_step_kernel<S, OUTER> (csrc/init.hip) in every compiled form against
the float64 model of tests/kmeans_reference.py -- bit for bit on the dyadic cases, within the bounds derived there on the
real-valued ones --, on row tiles, through the Lloyd driver and in the global covariance; argmax_kernel<VEC> (csrc/kernels.hip)
against np.argmax of the float32 rows; and the second grid-stride trip of all three kernels, emission_kernel included.
tests/test_kmeans_reference.py checks on the CPU that the cases and bounds are what they claim."""
import numpy as np
import pytest

from oracle import ref_numpy as R
from tests import kmeans_reference as KR

pytestmark = pytest.mark.gpu


def _block(n, S, K, X=None):
    from phylo_hmrf_amd import Block
    b = Block(n, S, K)
    if X is not None:
        b.set_observations(X)
    return b


def _call(b, entry, C, write_labels=True):
    """-> (labels or None, counts, sums, outer or None, inertia), the order of kmeans_reference.step"""
    if entry == "moments":
        sums, counts, inertia, outer = b.kmeans_moments(C, write_labels=write_labels)
    else:
        (sums, counts, inertia), outer = b.kmeans_step(C, write_labels=write_labels), None
    return (b.get_labels() if write_labels else None), counts, sums, outer, inertia


def _run_case(c):
    case = KR.case(*c)
    b = _block(case.n, case.S, case.K, case.X)
    got = _call(b, case.entry, case.C)
    b.close()
    figures = case.check(got)
    if figures:
        print("%s: labels that differ %d; error / bound: %s" % (KR.case_id(c), figures["labels"], ", ".join(
            "%s %.3f" % (k, v) for k, v in figures.items() if k != "labels")))


# ---- kmeans_step_kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", KR.FORM_CASES, ids=[KR.case_id(c) for c in KR.FORM_CASES])
def test_every_compiled_form(c):
    _run_case(c)


@pytest.mark.parametrize("c", KR.EDGE_CASES, ids=[KR.case_id(c) for c in KR.EDGE_CASES])
def test_tile_edges(c):
    _run_case(c)


@pytest.mark.parametrize("c", KR.TRIP_CASES, ids=[KR.case_id(c) for c in KR.TRIP_CASES])
def test_second_trip_of_the_grid_stride_loop(c):
    _run_case(c)


def _row_lengths(H, W, diag):
    return [W - r if diag else W for r in range(H)]


@pytest.mark.parametrize("top,bottom", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("H,W,diag", [(7, 40, False), (23, 23, True)])
def test_row_tiles_count_their_owned_rows_only(H, W, diag, top, bottom):
    rows = _row_lengths(H, W, diag)
    n = sum(rows)
    own = (rows[0] if top else 0, n - (rows[-1] if bottom else 0))           # all but the halo rows
    for S in (3, 4):
        X, C = KR.dyadic_case(np.random.default_rng([H, S, top, bottom]), n, S, 3)
        b = _block(n, S, 3, X)
        b.build_grid_graph(H, W, diag, 8, 0.5)
        b.set_tile(top, bottom)
        assert b.owned == own
        whole = KR.step(X, C)
        assert not np.array_equal(whole[1], KR.step(X, C, own)[1])           # (the halo rows do hold nodes that would count)
        for entry in ("step", "moments"):
            b.set_labels(np.zeros(n, dtype=np.int32))
            got = _call(b, entry, C)
            assert np.array_equal(got[0], whole[0])                          # every node is labelled, halo rows included
            KR.check_exact(X, C, got, own=own, with_outer=entry == "moments")
        b.set_tile(0, 0)
        assert b.owned == (0, n)
        for entry in ("step", "moments"):
            KR.check_exact(X, C, _call(b, entry, C), with_outer=entry == "moments")
        b.close()


@pytest.mark.parametrize("entry", ["step", "moments"])
def test_write_labels_false_leaves_the_labels(entry):
    n, S, K = 1300, 4, 7
    rng = np.random.default_rng(8)
    X, C = KR.dyadic_case(rng, n, S, K)
    before = rng.integers(0, K, n).astype(np.int32)
    b = _block(n, S, K, X)
    b.set_labels(before)
    quiet = _call(b, entry, C, write_labels=False)
    assert np.array_equal(b.get_labels(), before)
    KR.check_exact(X, C, quiet, with_outer=entry == "moments")
    loud = _call(b, entry, C, write_labels=True)
    assert np.array_equal(loud[0], KR.step(X, C)[0])
    assert all(np.array_equal(q, l) for q, l in zip(quiet[1:], loud[1:]) if q is not None)
    b.close()


ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5         # include/phmrf.h: PHMRF_ERR_INVALID, _UNSUPPORTED, _STATE


def _status(call, *args):
    from phylo_hmrf_amd import PhmrfError
    with pytest.raises(PhmrfError) as ei:
        call(*args)
    return ei.value.status


def test_no_observations_is_a_state_error():
    X, C = KR.dyadic_case(np.random.default_rng(4), 600, 3, 4)
    b = _block(600, 3, 4)
    assert _status(b.kmeans_step, C) == ERR_STATE and _status(b.kmeans_moments, C) == ERR_STATE
    b.set_observations(X)
    KR.check_exact(X, C, _call(b, "moments", C))
    b.close()


def test_a_non_finite_centre_is_invalid():
    X, C = KR.dyadic_case(np.random.default_rng(5), 600, 3, 4)
    b = _block(600, 3, 4, X)
    for bad in (np.nan, np.inf, -np.inf):
        Cb = C.copy()
        Cb[3, 2] = bad
        assert _status(b.kmeans_step, Cb) == ERR_INVALID and _status(b.kmeans_moments, Cb) == ERR_INVALID
    KR.check_exact(X, C, _call(b, "step", C), with_outer=False)          # (the block is still good)
    b.close()


def test_second_moments_at_nine_features_are_unsupported():
    b = _block(50, 9, 2, np.ones((50, 9)))
    assert _status(b.kmeans_moments, np.ones((2, 9))) == ERR_UNSUPPORTED
    assert b.kmeans_step(np.ones((2, 9)))[1][0] == 50
    b.close()


def test_emission_after_the_borrowed_parameter_buffer():
    """kmeans_* uploads its centres into the emission's parameter buffer: a later emission() must not see them"""
    from tests.test_gpu_estep import _emission_tol
    n, S, K = 600, 3, 4
    rng = np.random.default_rng(6)
    X, C = KR.dyadic_case(rng, n, S, K)
    mu = rng.uniform(0, 4, (K, S))
    A = rng.standard_normal((K, S, S))
    cov = np.einsum("kij,klj->kil", A, A) * 0.3 + 2e-3 * np.eye(S)
    ref = R.log_multivariate_normal_density_full(X, mu, cov)
    b = _block(n, S, K, X)
    b.emission(mu, cov)
    for entry in ("moments", "step"):
        KR.check_exact(X, C, _call(b, entry, C), with_outer=entry == "moments")
        b.emission(mu, cov)
        assert np.all(np.abs(b.get_logprob() - ref) <= _emission_tol(ref))
    b.close()


@pytest.mark.parametrize("ratio", [1, 10, 100])
def test_conditioning_of_the_global_covariance(ratio):
    """hmrf.py's first covariance, cv = (sum_k outer_k - n m m^T) / (n - 1) with m = sum_k sums_k / n, from the device's moments
    against np.cov of the same float32-valued rows, at mean / sd = 1, 10, 100.  The bound, entry (s, t), from kmeans_reference's:
      outer   E_o = sum_bound(sum |fl(x_s x_t)|) + u sum |x_s x_t|   (the second term: the products are rounded to f32 before
              they are summed, and np.cov squares in f64)
      sums    E_s = sum_bound(sum |x_s|): the mean term n m_s m_t moves by at most (|S_s| E_t + |S_t| E_s + E_s E_t) / n
      cv      (E_o + that) / (n - 1), and 1e-12 of (sum |x_s x_t| + |S_s S_t| / n) / (n - 1) for the float64 evaluation of
              both sides (the cancellation of the two large terms happens in float64 on both)
    The digits this keeps at each ratio are printed; DESIGN.md's paragraph "Initialisation, what the moments keep" records them next to the bound."""
    n, S, K = 50001, 4, 3
    rng = np.random.default_rng(ratio)
    sd = np.array([1.0, 0.5, 2.0, 1.5])
    X = KR.f32(ratio * sd + sd * rng.standard_normal((n, S)))
    C = KR.f32(ratio * sd + sd * rng.standard_normal((K, S)))
    b = _block(n, S, K, X)
    sums, counts, _, outer = b.kmeans_moments(C)
    b.close()
    assert counts.sum() == n
    n_tot = float(counts.sum())
    mean_all = sums.sum(axis=0) / n_tot
    cv = (outer.sum(axis=0) - n_tot * np.outer(mean_all, mean_all)) / (n_tot - 1.0)
    ref = np.cov(X.T)
    abs_o = np.abs(X[:, :, None] * X[:, None, :]).sum(axis=0)
    abs_s = np.abs(X).sum(axis=0)
    E_o = KR.sum_bound(abs_o * (1 + KR.U), n) + KR.U * abs_o
    E_s = KR.sum_bound(abs_s, n)
    St = np.abs(X.sum(axis=0))
    E_m = (np.outer(St, E_s) + np.outer(E_s, St) + np.outer(E_s, E_s)) / n
    bound = (E_o + E_m + 1e-12 * (abs_o + np.outer(St, St) / n)) / (n - 1.0)
    err = np.abs(cv - ref)
    var = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    print("mean/sd %3d: max |cv - np.cov| / bound %.3f; relative to sqrt(var_s var_t): measured %.2e (%.1f digits), bound %.2e"
          % (ratio, np.max(err / bound), np.max(err / var), -np.log10(np.max(err / var)), np.max(bound / var)))
    assert np.all(err <= bound)


def test_lloyd_driver_on_real_blocks():
    """test_kmeans.py's separated-blob case with three device blocks in place of the CPU doubles"""
    from phylo_hmrf_amd import kmeans
    from tests.test_kmeans import _blobs
    rng = np.random.default_rng(0)
    K, S = 6, 4
    X, truth, centers = _blobs(rng, K, S, 400)
    X = KR.f32(X)
    cuts = [0, 700, 1500, X.shape[0]]
    blocks = [_block(b - a, S, K, X[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    got, inertia = kmeans.device_kmeans(blocks, X[::3], K, np.random.default_rng(1))
    lab = np.concatenate([blk.get_labels() for blk in blocks])
    for blk in blocks:
        blk.close()
    d = np.sqrt(((centers[:, None, :] - got[None, :, :]) ** 2).sum(-1))
    assert np.all(d.min(axis=1) < 0.05)
    assert np.array_equal(d.argmin(axis=1)[truth], lab)                       # the partition is the truth
    # the device works on the centres rounded to float32; the inertia is the sum of three blocks' (each within its bound)
    Cf = KR.f32(got)
    assert np.array_equal(lab, KR.step(X, Cf)[0])
    ref = float(KR.distance_at(X, Cf, lab).sum())
    assert abs(inertia - ref) <= KR.inertia_bound(S, ref)


# ---- argmax_kernel -----------------------------------------------------------------------------------------------------
def _tile_threads(K):
    return 256 if K <= 40 else 128


def _argmax_rows(rng, n, K):
    """float32-valued rows with planted exact ties of the maximum (two and three columns, at either end) and all-equal rows"""
    lp = KR.f32(rng.normal(-5.0, 3.0, (n, K)))
    if K >= 2:
        kind = rng.integers(0, 4, n)
        top = lp.max(axis=1)
        r = np.arange(n)
        two = rng.integers(0, K, (n, 3))
        for j in range(2):
            m = kind == 1
            lp[r[m], two[m, j]] = top[m]                     # the maximum once or twice more, anywhere
        m = kind == 2
        lp[r[m], K - 1] = top[m]                              # ... and in the last column
        lp[kind == 3] = lp[kind == 3, :1]                     # all equal
    return lp


def _argmax_labels(b, lp):
    b.set_logprob(lp)
    b.set_labels(np.full(b.n, b.K - 1, dtype=np.int32))
    # solve_begin with init_mode = 1 and no coarse start runs the argmax initialiser and launches no move (a round's launches
    # are solve_round_launch's); solve_end without a result request evaluates nothing
    b.solve_begin(1.0, init_mode=1, coarse_start=0, use_chains=False, use_components=False, use_strips=False,
                  use_expansion=False, use_coarse=False)
    b.solve_end()
    return b.get_labels()


def _argmax_block(n, K):
    b = _block(n, 1, K)
    if n >= 2:
        b.set_graph(np.array([[0, 1]]), np.array([1.0]))
    else:
        b.set_graph(np.zeros((0, 2), dtype=np.int64), np.zeros(0))
    return b


@pytest.mark.parametrize("K", [1, 2, 3, 4, 7, 40, 41, 63, 64])
def test_argmax_initialiser(K):
    TB = _tile_threads(K)
    for n in (TB - 1, TB, TB + 1, 2 * TB + 1):
        lp = _argmax_rows(np.random.default_rng(K * 1000 + n), n, K)
        if K >= 2:
            top = lp == lp.max(axis=1, keepdims=True)
            assert np.count_nonzero(top.sum(axis=1) == 2) and np.count_nonzero(top.all(axis=1))
        b = _argmax_block(n, K)
        lab = _argmax_labels(b, lp)
        b.close()
        assert np.array_equal(lab, np.argmax(lp, axis=1)), (K, n)


TRIP_N2 = 4096 * 256 + 300             # grid_for caps the grid at 4096 workgroups of tile_threads(K) = 256 rows (K <= 40)


@pytest.mark.parametrize("K", [2, 4])
def test_argmax_second_trip(K):
    lp = _argmax_rows(np.random.default_rng(K), TRIP_N2, K)
    b = _argmax_block(TRIP_N2, K)
    lab = _argmax_labels(b, lp)
    b.close()
    bad = np.flatnonzero(lab != np.argmax(lp, axis=1))
    assert bad.size == 0, (bad.size, bad[:5])


# ---- emission_kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 4])
def test_emission_second_trip(K):
    """n above the grid cap: workgroups 0 and 1 take a second tile (the last one partial).  The rows against the float64 oracle;
    the label-major unary planes, which the emission kernel writes itself from a block's second E-step on, by the route of
    test_gpu_estep's test_unary_planes_written_by_the_emission_kernel: the grid energy reads them, and equals the energy of a
    block that holds the same rows only."""
    from tests.test_gpu_estep import _emission_tol
    H, W, S = 703, 1492, 2
    n = H * W
    assert n == TRIP_N2
    rng = np.random.default_rng(K)
    A = rng.standard_normal((K, S, S))
    cov = np.einsum("kij,klj->kil", A, A) * 0.3 + 2e-3 * np.eye(S)
    mu = rng.uniform(0, 4, (K, S))
    X = np.abs(mu[rng.integers(0, K, n)] + 0.7 * rng.standard_normal((n, S)))
    ref = R.log_multivariate_normal_density_full(X, mu, cov)
    a = _block(n, S, K, X)
    a.build_grid_graph(H, W, False, 8, 0.5)
    a.emission(mu, cov)
    lp = a.get_logprob()
    bad = np.abs(lp - ref) > _emission_tol(ref)
    assert not bad.any(), (np.count_nonzero(bad), np.argwhere(bad)[:3])
    labs = [rng.integers(0, K, n), np.arange(n) % K]
    a.set_labels(labs[0])
    a.strip_multi_pass(1.0, 0, 0, 0, labels=[0])          # the first strip move allocates the planes (transposed from the rows)
    a.emission(mu * 1.05, cov * 1.1)                      # the second emission writes rows and planes
    lp2 = a.get_logprob()
    ref2 = R.log_multivariate_normal_density_full(X, mu * 1.05, cov * 1.1)
    assert np.all(np.abs(lp2 - ref2) <= _emission_tol(ref2))
    c = _block(n, S, K, X)
    c.build_grid_graph(H, W, False, 8, 0.5)
    c.set_logprob(lp2)                                    # rows only: no planes, its energy reads the rows
    for lab in labs:
        a.set_labels(lab)
        c.set_labels(lab)
        ea, ec = a.energy(1.0), c.energy(1.0)
        assert abs(ea[1] - ec[1]) <= 1e-12 * abs(ec[1]) and abs(ea[2] - ec[2]) <= 1e-12 * abs(ec[2]), (ea, ec)
        host = -lp2[np.arange(n), lab].sum()
        assert abs(ea[1] - host) <= 1e-6 * abs(host)      # (test_gpu_estep's tolerance for the device's energy reduction)
    a.close()
    c.close()
