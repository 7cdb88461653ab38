"""GPU: the multi-label coarse sweep (solve.hip: coarse_sweep_nocount; coarse.hip: coarsen_kernel<S, NL>, the gated
one-label rebuild, coarse_apply_kernel) and the coarse-to-fine start kernels (c2f.hip) against float64 models:
oracle/mrf_moves.coarse_problem / coarse_sweep and tests/c2f_reference.py.  Inputs are dyadic (tests/coarse_sweep_cases.py), so
every comparison with a model is exact, except the one real-valued build, whose bound is worked out where it is used.  Every
test asserts from the model that its input does what it claims before it looks at the kernels."""
import numpy as np
import pytest

from oracle import mrf_moves as M
from oracle import ref_numpy as R
from tests import c2f_reference as F
from tests import coarse_sweep_cases as C
from tests.test_gpu_estep import _block

pytestmark = pytest.mark.gpu


def _setup(n, K, eid, w, H, W, diagonal, lp, labels):
    b = _block(n, 2, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 8)
    b.set_logprob(lp)
    if labels is not None:
        b.set_labels(labels)
    return b


# ------------------------------------------------------------------------------------------------ a. the batched build
@pytest.mark.parametrize("H,W,diagonal", C.BUILD_SHAPES)
@pytest.mark.parametrize("scale", [2, 4, 8])
def test_batched_build_matches_model_and_single_builds(H, W, diagonal, scale):
    """coarsen_kernel<scale, NL> for NL = 1, 2, 4 and three labels in a pass of four: every child's D and lam equal the model's
    per label, and -- bit for bit -- what one-label passes write ('the same numbers', coarse.hip).  Alphas: label 0, label
    K - 1, a label the labelling does not have, a label a whole super-cell carries."""
    K = C.BUILD_K
    n, eid, w, lp, lab = C.build_problem(H, W, diagonal)
    assert not (lab == 3).any() and (H < 19 or ((lab == 0).any() and (lab == K - 1).any()))
    g = M.Graph(n, eid, w)
    b = _setup(n, K, eid, w, H, W, diagonal, lp, lab)
    for off in C.BUILD_OFFSETS[scale]:
        cross = M.coarse_cross_weight(g, H, W, diagonal, scale, off)
        ref, single = {}, {}
        for alpha in (0, 2, 3, 4):
            ref[alpha] = M.coarse_problem(g, -lp, lab, 0.75, H, W, diagonal, scale, off, alpha)
            single[alpha] = b.coarse_problem(0.75, scale, off, alpha)
        if H >= 19:                 # (a whole super-cell of label 2: its switch to 2 is free and pulls on nobody)
            cnode = ref[2][2]
            full = [c for c in np.unique(cnode[lab == 2]) if np.all(lab[cnode == c] == 2)]
            assert full and np.all(ref[2][0][full] == 0.0) and np.all(ref[2][1][full] == 0.0)
        for nl in (1, 2, 3, 4):
            alphas = C.BUILD_ALPHAS[nl]
            D, lam = b.coarse_problems(0.75, scale, off, alphas)
            assert D.shape == (nl, len(cross)) and lam.shape == (nl, len(cross), 4)
            for q, alpha in enumerate(alphas):
                D_ref, lam_ref = ref[alpha][:2]
                pinned = D_ref > 0.75 * cross * 1.0001 + 1e-6
                assert np.array_equal(D[q] > 1e29, pinned), (off, nl, alpha)
                assert np.array_equal(D[q][~pinned].astype(np.float64), D_ref[~pinned]), (off, nl, alpha)
                assert np.array_equal(lam[q].astype(np.float64), lam_ref), (off, nl, alpha)
                assert lam[q].min() >= 0.0
                assert D[q].tobytes() == single[alpha][0].tobytes() and lam[q].tobytes() == single[alpha][1].tobytes()
    b.close()


def test_batched_build_real_valued():
    """synth.make_block 60 x 60 (upper triangle), K = 6, beta = 0.75, every scale, offset and batch size: the batch's arrays are
    the single builds' bit for bit, and every D and lam lies within the worst-case f32 bound of a sum in any order around the
    float64 problem of the same f32 inputs: T * 2^-23 * sum |terms| per super-cell, over the reference's own non-zero terms
    (tests/coarse_sweep_cases.problem_with_bounds; a D or lam without such a term, or with one, has to be exact).
    Super-cells whose float64 D lies within that bound of the pin threshold are left out of the pinned-mask comparison; at most
    1 % may be (none of the 7,788 are with this seed: tests/test_coarse_reference_cpu.py checks it with the host's emission).
    Observed on an MI355X, worst |error| / bound over all super-cells: D 0.291, lam 0.249 (printed below)."""
    blk, eid, w, lab = C.real_problem()
    X = blk["X"]
    n, K, H = X.shape[0], 6, 60
    b = _block(n, 4, K)
    b.set_observations(X)
    b.set_graph(eid, w)
    b.set_grid(H, H, True, 8)
    b.emission(blk["means"], blk["covars"])
    b.set_labels(lab)
    un32 = -b.get_logprob()                                        # (the f32 values, as float64)
    w32 = w.astype(np.float32).astype(np.float64)
    worst_D = worst_lam = 0.0
    left_out = total = 0
    for scale in (2, 4, 8):
        for off in C.BUILD_OFFSETS[scale]:
            single = [b.coarse_problem(C.REAL_BETA, scale, off, a) for a in range(K)]
            ref = [C.problem_with_bounds(eid, w32, un32, lab, C.REAL_BETA, H, H, True, scale, off, a) for a in range(K)]
            for alphas in ((5,), (1, 4), (0, 3, 2), (2, 5, 0, 1)):
                D, lam = b.coarse_problems(C.REAL_BETA, scale, off, alphas)
                for q, a in enumerate(alphas):
                    assert D[q].tobytes() == single[a][0].tobytes() and lam[q].tobytes() == single[a][1].tobytes()
            for a in range(K):
                D, lam = single[a]
                D_ref, lam_ref, bD, bl, thr, bt = ref[a]
                near = np.abs(D_ref - thr) <= bD + bt
                left_out += int(near.sum())
                total += len(D_ref)
                pinned = D_ref > thr
                assert np.array_equal((D > 1e29)[~near], pinned[~near]), (scale, off, a)
                free = D < 1e29
                err = np.abs(D[free].astype(np.float64) - D_ref[free])
                assert np.all(err <= bD[free]), (scale, off, a, float(np.max(err / np.maximum(bD[free], 1e-300))))
                errl = np.abs(lam.astype(np.float64) - lam_ref)
                assert np.all(errl <= bl), (scale, off, a)
                assert lam.min() >= 0.0
                if free.any() and bD[free].max() > 0:
                    worst_D = max(worst_D, float(np.max(err[bD[free] > 0] / bD[free][bD[free] > 0])))
                if (bl > 0).any():
                    worst_lam = max(worst_lam, float(np.max(errl[bl > 0] / bl[bl > 0])))
    print("worst error / bound: D %.4f, lam %.4f; left out %d of %d" % (worst_D, worst_lam, left_out, total))
    assert left_out <= 0.01 * total
    b.close()


# ------------------------------------------------------------------------------------------------ b. sweeps over a mask
@pytest.mark.parametrize("stamps", [0, 1])
@pytest.mark.parametrize("case", C.SWEEPS, ids=C.sweep_id)
def test_sweep_matches_the_one_by_one_model(case, stamps):
    """Precondition (asserted): from the random start, a sweep whose batches never rebuild ends in another labelling than
    the one-by-one sequence.  Then the labels, the changed total and the per-label counts of three sweeps on one block -- the
    second and third at other scales, offsets and cuts -- equal the model's."""
    H, W, diagonal, K, labels, steps = case
    m = C.sweep_model(case)
    assert int((m["stale"] != m["after"][0][0]).sum()) >= 100
    b = _setup(m["n"], K, m["eid"], m["w"], H, W, diagonal, m["lp"], m["init"])
    for it, (scale, off, sr, sc) in enumerate(steps):
        want, counts = m["after"][it]
        total, per = b.coarse_sweep(C.BETA, scale, off, labels, sr, sc, stamps=stamps)
        got = b.get_labels().astype(np.int64)
        assert np.array_equal(got, want), (it, int((got != want).sum()))
        assert np.array_equal(per, counts) and total == int(counts.sum()), (it, total, per, counts)
    b.close()


# ------------------------------------------------------------------------------------------------ c. constructed rebuilds
def _run_constructed(c, stamps=1):
    b = _setup(c.n, c.K, c.eid, c.w, c.H, c.W, c.diagonal, c.lp, c.init)
    total, per = b.coarse_sweep(C.BETA, c.scale, c.off, c.labels, c.cut[0], c.cut[1], stamps=stamps)
    got = b.get_labels().astype(np.int64)
    b.close()
    return got, total, per


@pytest.mark.parametrize("name", C.REBUILD_IDS)
def test_rebuild_crosses_wavefronts_workgroups_and_coarse_rows(name):
    """tests/coarse_sweep_cases.py: super-cell A takes label 1; its neighbour B -- across a wavefront's column boundary of
    the coarsen pass, across a workgroup's, in the coarse row below or above -- takes label 2 only in a problem rebuilt with
    A's move; T takes label 2 only in a stale problem.  Preconditions (asserted): d + w_B >= 0 > d + w_B - w_AB; the
    one-by-one labelling differs from the one without rebuilds; it differs from a rebuild of only the wavefronts that hold
    a CHANGED node (no stamps on the neighbours) in exactly B's nodes.  The sweep runs with change stamps."""
    c = C.rebuild_case(name)
    assert c.d_plus_wb >= 0 > c.d_plus_wb - c.w_ab
    fresh, counts = c.model()
    stale, _ = c.model(stale=True)
    undilated, _ = c.model(stale="waves")
    assert not np.array_equal(fresh, stale)
    assert np.array_equal(np.flatnonzero(undilated != fresh), np.sort(c.B))
    got, total, per = _run_constructed(c)
    assert np.array_equal(got, fresh), (int((got != fresh).sum()), bool(np.array_equal(got, stale)), bool(np.array_equal(got, undilated)))
    assert np.array_equal(per, counts) and total == int(counts.sum())


@pytest.mark.parametrize("stamps", [0, 1])
@pytest.mark.parametrize("name", C.MIRROR_IDS)
def test_rebuild_flag_down_then_up(name, stamps):
    """label 1 moves nothing, labels 2 and 3 move one super-cell each, far apart: the flag is down at label 2's rebuild and
    up at label 3's.  Precondition (asserted): the labelling without rebuilds IS the one-by-one labelling -- and the kernels,
    rebuilding for label 3, must still give it."""
    c = C.mirror_case(name)
    fresh, counts = c.model()
    stale, _ = c.model(stale=True)
    assert np.array_equal(fresh, stale) and counts[1] == 0 and counts[2] > 0 and counts[3] > 0
    got, total, per = _run_constructed(c, stamps)
    assert np.array_equal(got, fresh)
    assert np.array_equal(per, counts) and total == int(counts.sum())


@pytest.mark.parametrize("stamps", [0, 1])
@pytest.mark.parametrize("name", C.MIRROR_IDS)
def test_quiet_batch_changes_nothing(name, stamps):
    """Precondition (asserted): under the model no label of the batch switches any super-cell.  Every gate stays down: zero
    changes, total and per label, and the labels untouched."""
    c = C.quiet_case(name)
    lab, counts = c.model()
    assert counts.sum() == 0 and not lab.any()
    got, total, per = _run_constructed(c, stamps)
    assert total == 0 and not per.any() and not got.any()


# ------------------------------------------------------------------------------------------------ d. strided rows
@pytest.mark.parametrize("stamps", [0, 1])
@pytest.mark.parametrize("scale,off", C.STRIDED)
def test_strided_rows(scale, off, stamps):
    """8200 x 6, K = 3: one column of workgroups and more coarse rows (4101, 2051) and row groups of the apply pass (2050) than
    the 2048 workgroups a rebuild or a gated apply pass is given, so both run more than one row per workgroup.
    Precondition (asserted): under the model labels change in grid rows beyond 8192 and in coarse rows beyond 2048."""
    m = C.strided_model(scale, off)
    H, W, K = m["H"], m["W"], m["K"]
    assert (H - 1 + off) // scale + 1 > 2048 and (H + 3) // 4 > 2048 and (((W - 1 + off) // scale + 1) * scale + 255) // 256 == 1
    rows = np.flatnonzero(m["after"] != m["init"]) // W
    assert rows.max() >= 8192 and ((rows + off) // scale).max() >= 2048 and np.all(m["counts"] > 0)
    b = _setup(m["n"], K, m["eid"], m["w"], H, W, False, m["lp"], m["init"])
    total, per = b.coarse_sweep(C.BETA, scale, off, None, m["cut"][0], m["cut"][1], stamps=stamps)
    got = b.get_labels().astype(np.int64)
    b.close()
    assert np.array_equal(got, m["after"]), int((got != m["after"]).sum())
    assert np.array_equal(per, m["counts"]) and total == int(m["counts"].sum())


def test_sweep_refuses_to_run_inside_a_solve():
    from phylo_hmrf_amd import PhmrfError
    c = C.quiet_case("rect-s2o1")
    b = _setup(c.n, c.K, c.eid, c.w, c.H, c.W, c.diagonal, c.lp, c.init)
    b.solve_begin(1.0)
    with pytest.raises(PhmrfError) as ei:
        b.coarse_sweep(1.0, 2, 0)
    assert ei.value.status == 5
    b.solve_end()
    assert b.coarse_sweep(1.0, 2, 0, stamps=True)[0] == 0
    b.close()


# ------------------------------------------------------------------------------------------------ e. coarse-to-fine start
@pytest.mark.parametrize("H,W,diagonal", F.SHAPES)
@pytest.mark.parametrize("K", F.KS)
def test_c2f_child_problem_and_prolongation(H, W, diagonal, K):
    """c2f_graph_kernel, c2f_logprob_kernel, c2f_prolong_kernel against tests/c2f_reference.py: the child's rows (neighbours in
    the order NW N NE W E SW S SE, compacted, padded; summed crossing weights), its log-probabilities, and the labels and the
    energy of prolongated labellings -- all exact on dyadic inputs."""
    n, eid, w, lp = F.dyadic_inputs(3, H, W, K, diagonal)
    Hc_ref, Wc_ref, cnode, nbr_ref, wgt_ref, lpc_ref = F.c2f_problem(eid, w, lp, H, W, diagonal)
    b = _setup(n, K, eid, w, H, W, diagonal, lp, None)
    Hc, Wc, nbr, wgt, lpc = b.c2f_problem()
    assert (Hc, Wc) == (Hc_ref, Wc_ref) and nbr.shape == nbr_ref.shape
    assert np.array_equal(nbr.astype(np.int64), nbr_ref)
    assert np.array_equal(wgt.astype(np.float64), wgt_ref)
    assert np.array_equal(lpc.astype(np.float64), lpc_ref)
    for C0 in range(nbr.shape[0]):                   # symmetric: wgt[C -> C'] == wgt[C' -> C]
        for q in range(8):
            if nbr[C0, q] >= 0:
                back = np.flatnonzero(nbr[nbr[C0, q]] == C0)
                assert len(back) == 1 and wgt[nbr[C0, q], back[0]] == wgt[C0, q]
    eid_c, w_c = F.coarse_edges(nbr_ref, wgt_ref)
    rng = np.random.default_rng(H + K)
    for beta in (1.0, 0.5, 2.0):
        lc = rng.integers(0, K, nbr.shape[0])
        b.c2f_prolong(lc)
        assert np.array_equal(b.get_labels().astype(np.int64), lc[cnode])
        assert b.energy(beta) == R.mrf_energy(lc, lpc_ref, eid_c, w_c, beta)
    b.close()


def test_c2f_entries_keep_the_conditions_of_the_start():
    from phylo_hmrf_amd import PhmrfError
    n, eid, w, lp = F.dyadic_inputs(3, 33, 33, 2, True)            # n = 561 < 1024
    b = _setup(n, 2, eid, w, 33, 33, True, lp, None)
    n2, eid2, w2, lp2 = F.dyadic_inputs(3, 32, 33, 2, False)
    gone = len(eid2) // 2
    b2 = _setup(n2, 2, np.delete(eid2, gone, axis=0), np.delete(w2, gone), 32, 33, False, lp2, None)     # a missing edge
    for blk, nc in ((b, 45), (b2, 72)):
        with pytest.raises(PhmrfError) as ei:
            blk.c2f_problem()
        assert ei.value.status == 5
        with pytest.raises(PhmrfError) as ei:
            blk.c2f_prolong(np.zeros(nc, dtype=np.int64))
        assert ei.value.status == 5
        blk.close()
