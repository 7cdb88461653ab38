"""CPU: the float64 models behind the coarse-sweep and coarse-to-fine tests, checked against each other -- the split of
coarse_expansion, the sweep model and its deliberately wrong variants (oracle/mrf_moves.py), the child problem of the
coarse-to-fine start (tests/c2f_reference.py) -- and the preconditions of the constructed cases
(tests/coarse_sweep_cases.py), which tests/test_gpu_coarse_sweep.py asserts again before it looks at a kernel."""
import numpy as np
import pytest

from oracle import mrf_moves as M
from oracle import ref_numpy as R
from tests import c2f_reference as F
from tests import coarse_sweep_cases as C
from tests.test_gpu_estep import _integer_problem


# ------------------------------------------------------------------------------------------------ coarse-to-fine reference
@pytest.mark.parametrize("H,W,diagonal", F.SHAPES)
@pytest.mark.parametrize("K", F.KS)
def test_c2f_reference_keeps_the_energy_of_labellings_constant_on_super_cells(H, W, diagonal, K):
    """the reason the child problem exists: E_fine(prolongation of L) == E_coarse(L), exactly on dyadic inputs"""
    n, eid, w, lp = F.dyadic_inputs(3, H, W, K, diagonal)
    Hc, Wc, cnode, nbr, wgt, lpc = F.c2f_problem(eid, w, lp, H, W, diagonal)
    nc = lpc.shape[0]
    assert (Hc, Wc) == (-(-H // 4), -(-W // 4)) and nc == (Hc * (Hc + 1) // 2 if diagonal else Hc * Wc)
    assert np.array_equal(np.bincount(cnode, minlength=nc) > 0, np.ones(nc, dtype=bool))
    eid_c, w_c = F.coarse_edges(nbr, wgt)
    # rows are symmetric, compacted and padded
    for C0 in range(nc):
        k = int((nbr[C0] >= 0).sum())
        assert np.all(nbr[C0, :k] >= 0) and np.all(nbr[C0, k:] == -1) and np.all(wgt[C0, k:] == 0.0)
        for q in range(k):
            back = np.flatnonzero(nbr[nbr[C0, q]] == C0)
            assert len(back) == 1 and wgt[nbr[C0, q], back[0]] == wgt[C0, q]
    rng = np.random.default_rng(K)
    for beta in (1.0, 0.5):
        lc = rng.integers(0, K, nc)
        assert R.mrf_energy(lc[cnode], lp, eid, w, beta) == R.mrf_energy(lc, lpc, eid_c, w_c, beta)


@pytest.mark.parametrize("H,W,diagonal", F.SHAPES)
def test_c2f_reference_with_two_directions_swapped_is_another_problem(H, W, diagonal):
    """the check of the GPU test itself: a crossing weight in the wrong one of the eight neighbours (here N and W, or NE and
    SW, exchanged) changes the rows at every shape the GPU test compares"""
    n, eid, w, lp = F.dyadic_inputs(3, H, W, 2, diagonal)
    ref = F.c2f_problem(eid, w, lp, H, W, diagonal)
    for a, b in ((1, 3), (2, 5)):
        d = list(F.DIRECTIONS)
        d[a], d[b] = d[b], d[a]
        bad = F.c2f_problem(eid, w, lp, H, W, diagonal, directions=tuple(d))
        assert not (np.array_equal(bad[3], ref[3]) and np.array_equal(bad[4], ref[4]))


# ------------------------------------------------------------------------------------------------ the sweep model
@pytest.mark.parametrize("H,W,K,diagonal,s,off", [(20, 70, 5, False, 2, 1), (40, 40, 4, True, 4, 3), (17, 66, 3, False, 8, 5)])
def test_coarse_sweep_is_a_loop_of_coarse_expansions(H, W, K, diagonal, s, off):
    n, eid, w, lp, init = _integer_problem(21, H, W, K, diagonal)
    g = M.Graph(n, eid, w)
    a, b, c, d = (init.astype(np.int64).copy() for _ in range(4))
    want = [M.coarse_expansion(g, -lp, a, 1.0, H, W, diagonal, s, off, alpha, 2, 40) for alpha in range(K)]
    got = M.coarse_sweep(g, -lp, b, 1.0, H, W, diagonal, s, off, list(range(K)), 2, 40)
    assert got == want and np.array_equal(a, b) and sum(want) > 0
    # the two halves of coarse_expansion, called one after the other
    halves = []
    for alpha in range(K):
        D, lam, cnode, Hc, Wc = M.coarse_problem(g, -lp, c, 1.0, H, W, diagonal, s, off, alpha)
        halves.append(M.coarse_solve_apply(D, lam, cnode, Hc, Wc, c, 1.0, diagonal, alpha, 2, 40))
    assert halves == want and np.array_equal(a, c)
    # a rebuild restricted to the wavefronts that hold a changed node OR A NEIGHBOUR of one loses nothing (the kernel's gate)
    gated = M.coarse_sweep(g, -lp, d, 1.0, H, W, diagonal, s, off, list(range(K)), 2, 40, stale="waves-dilated")
    assert gated == want and np.array_equal(a, d)


@pytest.mark.parametrize("case", C.SWEEPS, ids=C.sweep_id)
def test_random_sweeps_notice_a_missing_rebuild(case):
    """precondition of the random sweeps: from the random start a sweep that never rebuilds ends in another labelling"""
    m = C.sweep_model(case)
    assert int((m["stale"] != m["after"][0][0]).sum()) >= 100


@pytest.mark.parametrize("scale,off", C.STRIDED)
def test_strided_rows_case_meets_its_precondition(scale, off):
    """8200 x 6: one column of workgroups, more coarse rows and apply row groups than 2048, and under the model labels change
    in grid rows beyond 8192 and in coarse rows beyond 2048, for every label"""
    m = C.strided_model(scale, off)
    H, W = m["H"], m["W"]
    assert (H - 1 + off) // scale + 1 > 2048 and (H + 3) // 4 > 2048 and (((W - 1 + off) // scale + 1) * scale + 255) // 256 == 1
    rows = np.flatnonzero(m["after"] != m["init"]) // W
    assert rows.max() >= 8192 and ((rows + off) // scale).max() >= 2048 and np.all(m["counts"] > 0)


# ------------------------------------------------------------------------------------------------ constructed cases
@pytest.mark.parametrize("name", C.REBUILD_IDS)
def test_rebuild_cases_meet_their_preconditions(name):
    """A moves under label 1, B under label 2 only in a problem rebuilt with A's move, T under label 2 only in a stale one:
    one-by-one != never rebuilt; one-by-one != rebuilt without the stamps on a changed node's neighbours, and these two
    differ in exactly B's nodes; with those stamps the rebuild is complete"""
    c = C.rebuild_case(name)
    assert c.d_plus_wb >= 0 > c.d_plus_wb - c.w_ab
    fresh, cnt = c.model()
    assert np.all(fresh[c.A] == 1) and np.all(fresh[c.B] == 2) and np.all(fresh[c.T] == 1)
    assert cnt[1] == len(c.A) + len(c.T) and cnt[2] == len(c.B) and cnt.sum() == cnt[1] + cnt[2]
    stale, _ = c.model(stale=True)
    assert np.all(stale[c.B] == 0) and np.all(stale[c.T] == 2) and not np.array_equal(stale, fresh)
    undilated, _ = c.model(stale="waves")
    assert np.array_equal(np.flatnonzero(undilated != fresh), np.sort(c.B))
    dilated, cnt_d = c.model(stale="waves-dilated")
    assert np.array_equal(dilated, fresh) and np.array_equal(cnt_d, cnt)


@pytest.mark.parametrize("name", C.MIRROR_IDS)
def test_mirror_and_quiet_cases_meet_their_preconditions(name):
    c = C.mirror_case(name)
    fresh, cnt = c.model()
    stale, cnt_s = c.model(stale=True)
    assert np.array_equal(fresh, stale) and np.array_equal(cnt, cnt_s)
    assert cnt[1] == 0 and cnt[2] == c.scale ** 2 and cnt[3] == c.scale ** 2
    q = C.quiet_case(name)
    lab, cnt = q.model()
    assert cnt.sum() == 0 and not lab.any()


def test_real_valued_build_keeps_clear_of_the_pin_threshold():
    """the one real-valued case of the GPU test (batched build, 60 x 60, K = 6): with the reference alone -- the host's
    emission rounded to f32 -- at most 1 % of the super-cells have a D within the f32 bound of the pin threshold (they are
    left out of the pinned-mask comparison); the bounds are those of sums of non-negative magnitudes"""
    blk, eid, w, lab = C.real_problem()
    lp = R.log_multivariate_normal_density_full(blk["X"], blk["means"], blk["covars"]).astype(np.float32).astype(np.float64)
    w32 = w.astype(np.float32).astype(np.float64)
    near = total = 0
    for scale in (2, 4, 8):
        for off in C.BUILD_OFFSETS[scale]:
            for alpha in range(6):
                D, lam, bD, bl, thr, bt = C.problem_with_bounds(eid, w32, -lp, lab, C.REAL_BETA, 60, 60, True, scale, off, alpha)
                assert np.all(bD >= 0) and np.all(bl >= 0) and lam.min() >= 0
                near += int((np.abs(D - thr) <= bD + bt).sum())
                total += len(D)
    assert total == 7788 and near <= 0.01 * total
