"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against
 (1) the golden fixtures recorded from the reference, (2) the float64 oracle on seeded inputs,
 (3) the reference's gco labellings (energy parity), (4) size-independent properties.

Tolerances (stated here, used below):
  emission      |lp_gpu - lp_ref| <= 2e-6 * |lp_ref| + 2e-4     (f32 device arithmetic vs f64 oracle;
                near-singular covariances with only the 2e-3 jitter amplify f32 rounding of x - mu)
  posteriors    abs 2e-5;   statistics rel 2e-5;   cost scalars rel 1e-5
  energy        device f64 reduction vs oracle: rel 1e-6 (logprob is stored in f32)
"""
import os

import numpy as np
import pytest

from oracle import mrf_moves as M
from oracle import ref_numpy as R
from oracle import synth
from tests.fixed_point_audit import segment_chain_model as _segment_chain_model

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _block(n, S, K):
    from phylo_hmrf_amd import Block
    return Block(n, S, K)


def _emission_tol(ref):
    return 2e-6 * np.abs(ref) + 2e-4


# ------------------------------------------------------------------------------------------------ b1
@pytest.mark.parametrize("tag", ["s4", "s8"])
def test_emission_golden(tag):
    g = np.load(os.path.join(G, "emission.npz"))
    X, mu, cov, ref = g[tag + "_X"], g[tag + "_means"], g[tag + "_covars"], g[tag + "_logprob"]
    b = _block(X.shape[0], X.shape[1], mu.shape[0])
    b.set_observations(X)
    b.emission(mu, cov)
    lp = b.get_logprob()
    assert np.all(np.abs(lp - ref) <= _emission_tol(ref)), np.max(np.abs(lp - ref) / (1 + np.abs(ref)))
    b.close()


@pytest.mark.parametrize("S,K,n", [(4, 10, 70001), (4, 20, 4099), (8, 30, 5000), (3, 7, 1000), (4, 64, 777), (1, 1, 5),
                                   (2, 9, 1031), (5, 64, 517), (6, 11, 1031), (7, 64, 517), (9, 13, 1031), (12, 64, 517), (16, 15, 1031),
                                   (2, 64, 300), (6, 64, 300), (9, 64, 300), (16, 64, 300), (5, 5, 1031), (7, 3, 1031), (12, 7, 1031)])
def test_emission_oracle_shapes(S, K, n):
    rng = np.random.default_rng(S * 100 + K)
    A = rng.standard_normal((K, S, S))
    cov = np.einsum("kij,klj->kil", A, A) * 0.3 + 2e-3 * np.eye(S)
    mu = rng.uniform(0, 4, (K, S))
    X = np.abs(mu[rng.integers(0, K, n)] + 0.7 * rng.standard_normal((n, S)))
    ref = R.log_multivariate_normal_density_full(X, mu, cov)
    b = _block(n, S, K)
    b.set_observations(X)
    b.emission(mu, cov)
    lp = b.get_logprob()
    assert np.all(np.abs(lp - ref) <= _emission_tol(ref)), np.max(np.abs(lp - ref) / (1 + np.abs(ref)))
    b.close()


def test_emission_not_positive_definite_is_an_error():
    from phylo_hmrf_amd import PhmrfError
    b = _block(10, 2, 2)
    b.set_observations(np.ones((10, 2)))
    cov = np.array([[[1.0, 2.0], [2.0, 1.0]], [[1.0, 0.0], [0.0, 1.0]]])
    with pytest.raises(PhmrfError) as ei:
        b.emission(np.zeros((2, 2)), cov)
    assert ei.value.status == 6
    b.close()


def test_emission_ou_params_golden_chain():
    """params -> (means, covars) by the oracle recursion (pinned by tests/golden/ou_params.npz), then the GPU."""
    g1 = np.load(os.path.join(G, "tree_tables.npz"))
    g = np.load(os.path.join(G, "ou_params.npz"))
    tt = R.TreeTables(g1["t4_edge_list"])
    means, covars = g["t4_means"], g["t4_covars"] + 1e-3 * np.eye(4)
    rng = np.random.default_rng(5)
    X = np.abs(means[rng.integers(0, 5, 3000)] + 0.5 * rng.standard_normal((3000, 4)))
    ref = R.log_multivariate_normal_density_full(X, means, covars)
    b = _block(3000, 4, 5)
    b.set_observations(X)
    b.emission(means, covars)
    lp = b.get_logprob()
    assert np.all(np.abs(lp - ref) <= _emission_tol(ref))
    b.close()


# ------------------------------------------------------------------------------------------------ b2
def _integer_problem(seed, H, W, K, diagonal):
    """Unaries and weights are small integers / dyadic rationals: f32 arithmetic is exact, so the GPU moves must
    reproduce the float64 move model label for label.  Unaries are multiples of 0.5 and weights multiples of 1/8, so with
    beta in BETAS every term is a multiple of 1/16; a strip's sums stay below 315 cells x 24 < 2^13 and a whole block's
    below 2^20 sixteenths: exact in f32 and in the 2^-16 fixed point of the deterministic component table."""
    rng = np.random.default_rng(seed)
    n = H * (H + 1) // 2 if diagonal else H * W
    X = rng.uniform(0.5, 2, (n, 2))
    e = R.grid_edges(X, H, W, diagonal, 8)
    eid = np.int64(e[:, :2])
    w = rng.integers(1, 9, len(eid)) / 8.0
    img = synth.label_image(rng, H, W, K, mean_run=6)
    if diagonal:
        ii, jj = np.triu_indices(H)
        truth = img[ii, jj]
    else:
        truth = img.reshape(-1)
    un = rng.integers(0, 12, (n, K)).astype(np.float64) * 0.5
    un[np.arange(n), truth] -= 2.0
    init = rng.integers(0, K, n)
    return n, eid, w, -un, init


BETAS = (0.5, 1.0, 2.0)


def _as_before(*values):
    """a case that existed before the tests took (seed, beta, cuts, variant): it keeps its id"""
    return pytest.param(*values, id="-".join(str(v) for v in values[:4]))


# Shapes that put a strip's end on the edges of its 63-column window and its 5-row band, and the cuts that go with them
# (the window's first and last shift, one off either): every shape runs every cut in both orientations.
EDGE_SHAPES = [(12, 63, False), (12, 64, False), (12, 65, False), (12, 127, False), (12, 128, False), (5, 70, False),
               (6, 70, False), (7, 70, False), (11, 70, False), (63, 63, True), (64, 64, True), (65, 65, True)]
EDGE_CUTS = [(0, 0), (5, 63), (1, 1), (4, 62)]
# (seeds 4, 6, 11 and the three betas dealt over the shapes)
EDGE_CASES = [(H, W, 3, diag, (4, 6, 11)[i % 3], BETAS[(i // 3 + i) % 3], "edge", "plain") for i, (H, W, diag) in enumerate(EDGE_SHAPES)]


def _variant(variant, n, K, w, init):
    """the degenerate inputs of the strip tests"""
    if variant == "zero weights":          # every node independent: the per-node argmin, ties to the current label
        return np.zeros_like(w), init
    if variant == "constant":              # one label everywhere, label K - 1 absent
        return w, np.full(n, min(1, K - 2))
    assert variant == "plain"
    return w, init


MULTI_CASES = [_as_before(H, W, K, d, 6, 1.0, "std", "plain") for H, W, K, d in
               [(23, 70, 4, False), (41, 41, 6, True), (6, 200, 3, False), (130, 7, 5, False), (64, 129, 20, False),
                (3, 3, 2, True), (30, 66, 64, False), (35, 35, 30, True)]]
MULTI_CASES += [(23, 70, 4, False, 4, 0.5, "std", "plain"), (41, 41, 6, True, 11, 2.0, "std", "plain"),
                (30, 66, 64, False, 4, 0.5, "std", "plain"), (23, 70, 4, False, 6, 2.0, "std", "zero weights"),
                (41, 41, 6, True, 6, 0.5, "std", "constant")] + EDGE_CASES


@pytest.mark.parametrize("H,W,K,diagonal,seed,beta,cuts,variant", MULTI_CASES)
def test_strip_multi_pass_matches_the_single_label_passes(H, W, K, diagonal, seed, beta, cuts, variant):
    """strip_cols_kernel (every label of a cut in one launch, behind the exact filter) = the strip alpha-expansions of
    the move model applied label after label, label for label -- the filter loses no move and breaks no tie differently."""
    n, eid, w, lp, init = _integer_problem(seed, H, W, K, diagonal)
    w, init = _variant(variant, n, K, w, init)
    g = M.Graph(n, eid, w)
    b = _block(n, 2, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 8)
    b.set_logprob(lp)
    b.set_labels(init)
    lab = init.astype(np.int64).copy()
    total = 0
    passes = [(0, 0, 0, None), (1, 3, 17, None), (0, 2, 40, [K - 1, 0]), (1, 5, 63, None), (0, 4, 21, None), (1, 0, 42, None)]
    if cuts == "edge":
        passes = [(orient, sr, sc, None) for sr, sc in EDGE_CUTS for orient in (0, 1)]
    for it, (orient, sr, sc, labels) in enumerate(passes):
        ch_ref = 0
        for alpha in (range(K) if labels is None else sorted(labels)):
            ch_ref += M.strip_fusion(g, -lp, lab, np.full(n, alpha), beta, H, W, diagonal, orient, sr, sc)
        ch = b.strip_multi_pass(beta, orient, sr, sc, labels)
        got = b.get_labels().astype(np.int64)
        assert np.array_equal(got, lab), (it, int((got != lab).sum()))
        assert ch == ch_ref
        total += ch
    assert total > 0 or n < 20
    if variant == "zero weights" and cuts == "std":
        # independent nodes: whatever lay inside a strip of some pass is at its own argmin, or tied with it
        un = -lp
        assert np.mean(un[np.arange(n), lab] == un.min(axis=1)) > 0.9
    b.close()


@pytest.mark.parametrize("H,W,K,diagonal,beta", [_as_before(37, 37, 5, True, 1.0), _as_before(30, 45, 8, False, 1.0),
                                                 _as_before(70, 70, 20, True, 1.0), _as_before(9, 200, 3, False, 1.0),
                                                 (37, 37, 5, True, 0.5), (30, 45, 8, False, 2.0)])
def test_icm_sweep_matches_move_model(H, W, K, diagonal, beta):
    n, eid, w, lp, init = _integer_problem(1, H, W, K, diagonal)
    g = M.Graph(n, eid, w)
    col, nc = M.icm_colours(H, W, diagonal)
    b = _block(n, 2, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 8)
    b.set_logprob(lp)
    b.set_labels(init)
    lab = init.astype(np.int64).copy()
    for sweep in range(3):
        ch_ref = M.icm_sweep(g, -lp, lab, beta, col, nc)
        ch = b.icm_sweep(beta)
        assert ch == ch_ref
        assert np.array_equal(b.get_labels(), lab)
    e = b.energy(beta)
    np.testing.assert_allclose(e[0], M.energy(g, -lp, lab, beta)[0], rtol=1e-9)
    b.close()


def test_icm_general_graph_greedy_colouring_never_raises_energy():
    rng = np.random.default_rng(3)
    n, K = 5000, 6
    a = rng.integers(0, n, 15000)
    c = rng.integers(0, n, 15000)
    keep = a != c
    pairs = np.unique(np.stack([np.minimum(a, c)[keep], np.maximum(a, c)[keep]], 1), axis=0)
    w = rng.uniform(0, 1, len(pairs))
    lp = -rng.uniform(0, 5, (n, K))
    g = M.Graph(n, pairs, w)
    b = _block(n, 2, K)
    b.set_graph(pairs, w)
    b.set_logprob(lp)
    b.set_labels(rng.integers(0, K, n))
    prev = b.energy(1.0)[0]
    for _ in range(6):
        b.icm_sweep(1.0)
        e = b.energy(1.0)[0]
        assert e <= prev + 1e-6 * abs(prev)
        prev = e
    np.testing.assert_allclose(prev, M.energy(g, -lp, b.get_labels().astype(np.int64), 1.0)[0], rtol=1e-6)
    b.close()


@pytest.mark.parametrize("H,W,K,diagonal,beta", [_as_before(40, 40, 5, True, 1.0), _as_before(33, 150, 8, False, 1.0),
                                                 _as_before(130, 130, 20, True, 1.0), (40, 40, 5, True, 0.5),
                                                 (33, 150, 8, False, 2.0), (40, 40, 64, True, 1.0), (20, 70, 33, False, 2.0)])
def test_chain_sweeps_match_move_model(H, W, K, diagonal, beta):
    """A family's sweep (two colours, both segment cuts) ends at the model's energy.  The later colours and cuts start
    from what the earlier ones wrote, so kernel and model must also break exact ties alike: both keep a segment's labelling
    when it already attains the minimum (oracle/mrf_moves.py, the chain move's tie rule).  A model without that rule parts
    from the kernel at the first tie and ends the family elsewhere (33 x 150, family 1: 5918.5 against 5921.125)."""
    n, eid, w, lp, init = _integer_problem(2, H, W, K, diagonal)
    g = M.Graph(n, eid, w)
    b = _block(n, 2, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 8)
    b.set_logprob(lp)
    b.set_labels(init)
    lab = init.astype(np.int64).copy()
    for family in range(4):
        ch_ref = _segment_chain_model(g, -lp, lab, beta, H, W, diagonal, family, 0)
        ch_ref += _segment_chain_model(g, -lp, lab, beta, H, W, diagonal, family, 1)
        ch = b.chain_sweep(beta, family)
        got = b.get_labels()
        e_gpu = M.energy(g, -lp, got.astype(np.int64), beta)[0]
        e_ref = M.energy(g, -lp, lab, beta)[0]
        # integer problem: exact arithmetic; ties may be broken differently only if the energies are equal
        assert abs(e_gpu - e_ref) < 1e-9, (family, e_gpu, e_ref)
        lab = got.astype(np.int64).copy()
    b.close()


PASS_CASES = [_as_before(H, W, K, d, 4, 1.0, "std", "plain") for H, W, K, d in
              [(23, 70, 4, False), (41, 41, 6, True), (6, 200, 3, False), (130, 7, 5, False)]]
# (the fusion pass behind the filter at the two large label counts; the other betas and seeds; the degenerate inputs)
PASS_CASES += [(64, 129, 20, False, 4, 1.0, "std", "plain"), (30, 66, 64, False, 6, 0.5, "std", "plain"),
               (23, 70, 4, False, 6, 0.5, "std", "plain"), (41, 41, 6, True, 11, 2.0, "std", "plain"),
               (23, 70, 4, False, 11, 2.0, "std", "zero weights"), (41, 41, 6, True, 4, 0.5, "std", "constant")] + EDGE_CASES


@pytest.mark.parametrize("H,W,K,diagonal,seed,beta,cuts,variant", PASS_CASES)
def test_strip_passes_match_move_model(H, W, K, diagonal, seed, beta, cuts, variant):
    n, eid, w, lp, init = _integer_problem(seed, H, W, K, diagonal)
    w, init = _variant(variant, n, K, w, init)
    g = M.Graph(n, eid, w)
    b = _block(n, 2, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 8)
    b.set_logprob(lp)
    b.set_labels(init)
    lab = init.astype(np.int64).copy()
    passes = [(0, 0, 0, -1), (1, 3, 17, -1), (0, 2, 40, 1), (1, 5, 63, 0), (0, 4, 5, -1)]
    if cuts == "edge":       # every cut in both orientations, the fusion pass and a single label's expansion taking turns
        passes = [(orient, sr, sc, -1 if (i + orient) % 2 == 0 else (i + orient) % K)
                  for i, (sr, sc) in enumerate(EDGE_CUTS) for orient in (0, 1)]
        passes += [(orient, sr, sc, -1 if (i + orient) % 2 else (i + orient) % K)
                   for i, (sr, sc) in enumerate(EDGE_CUTS) for orient in (0, 1)]
    for it, (orient, sr, sc, alpha) in enumerate(passes):
        prop = M.best_alternative(g, -lp, lab, beta) if alpha < 0 else np.full(n, alpha)
        ch_ref = M.strip_fusion(g, -lp, lab, prop, beta, H, W, diagonal, orient, sr, sc)
        ch = b.strip_pass(beta, orient, sr, sc, alpha)
        got = b.get_labels().astype(np.int64)
        e_gpu, e_ref = M.energy(g, -lp, got, beta)[0], M.energy(g, -lp, lab, beta)[0]
        assert abs(e_gpu - e_ref) < 1e-9, (it, e_gpu, e_ref)      # exact arithmetic: same optimum value
        assert np.array_equal(got, lab), (it, int((got != lab).sum()))
        assert ch == ch_ref
    b.close()


@pytest.mark.parametrize("H,W,K,diagonal,beta", [_as_before(30, 45, 4, False, 1.0), _as_before(50, 50, 7, True, 1.0),
                                                 (30, 45, 4, False, 0.5), (50, 50, 7, True, 2.0)])
def test_component_pass_matches_move_model(H, W, K, diagonal, beta):
    n, eid, w, lp, init = _integer_problem(6, H, W, K, diagonal)
    g = M.Graph(n, eid, w)
    b = _block(n, 2, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 8)
    b.set_logprob(lp)
    lab = init.astype(np.int64).copy()
    col, nc = M.icm_colours(H, W, diagonal)
    for _ in range(3):                       # a few ICM sweeps give blobs worth relabelling
        M.icm_sweep(g, -lp, lab, beta, col, nc)
    b.set_labels(lab)
    for it in range(3):
        ch_ref = M.component_pass(g, -lp, lab, beta)
        ch = b.component_pass(beta)
        assert np.array_equal(b.get_labels(), lab), it
        assert ch == ch_ref
    b.close()


def test_moves_never_raise_energy_and_solver_converges():
    blk = synth.make_block(11, 90, 90, 4, 10, True)
    X = blk["X"]
    n = X.shape[0]
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    b = _block(n, 4, 10)
    b.set_observations(X)
    b.set_graph(eid, w)
    b.set_grid(90, 90, True, 8)
    b.emission(blk["means"], blk["covars"])
    rng = np.random.default_rng(0)
    b.set_labels(rng.integers(0, 10, n))
    prev = b.energy(1.0)[0]
    for rnd in range(3):
        for fam in range(4):
            b.chain_sweep(1.0, fam)
            e = b.energy(1.0)[0]
            assert e <= prev + 1e-6 * abs(prev), ("chain", fam, e, prev)
            prev = e
        b.icm_sweep(1.0)
        e = b.energy(1.0)[0]
        assert e <= prev + 1e-6 * abs(prev)
        prev = e
        b.component_pass(1.0)
        e = b.energy(1.0)[0]
        assert e <= prev + 1e-6 * abs(prev), ("component", e, prev)
        prev = e
        for orient in (0, 1):
            for alpha in (-1, rnd):
                b.strip_pass(1.0, orient, (2 * rnd + orient) % 6, (11 * rnd) % 64, alpha)
                e = b.energy(1.0)[0]
                assert e <= prev + 1e-6 * abs(prev), ("strip", orient, alpha, e, prev)
                prev = e
    res = b.solve(1.0)
    assert res["converged"]
    assert res["energy"] <= prev + 1e-6 * abs(prev)
    # idempotence: solving again from the fixed point changes nothing
    res2 = b.solve(1.0)
    assert res2["changed"] == 0 and res2["rounds"] == 2          # one ordinary round + the verification round
    b.close()


@pytest.mark.parametrize("H,W,diagonal", [(70, 70, True), (37, 90, False)])
def test_unary_planes_written_by_the_emission_kernel(H, W, diagonal):
    """From a block's second E-step on, the emission kernel writes the label-major unary planes itself and the grid
    energy, the proposals and the strip moves read them: same energy as from the node-major rows, same solve as a
    block that transposes the rows."""
    blk = synth.make_block(3, H, W, 4, 6, diagonal)
    X = blk["X"]
    n = X.shape[0]
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    rng = np.random.default_rng(1)
    init = rng.integers(0, 6, n)
    means2, covars2 = blk["means"] * 1.05, blk["covars"] * 1.1

    def fresh():
        b = _block(n, 4, 6)
        b.set_observations(X)
        b.set_graph(eid, w)
        b.set_grid(H, W, diagonal, 8)
        return b

    a = fresh()
    a.emission(blk["means"], blk["covars"])
    a.set_labels(init)
    a.solve(1.0)                                   # first solve: the planes are allocated and transposed from the rows
    a.emission(means2, covars2)                    # second emission: the kernel writes rows and planes
    a.set_labels(init)
    e_planes = a.energy(1.0)
    lp = a.get_logprob()
    ra = a.solve(1.0)
    la = a.get_labels()
    b = fresh()
    b.set_logprob(lp)                              # rows only: energy from the rows, planes by the transpose kernel
    b.set_labels(init)
    e_rows = b.energy(1.0)
    rb = b.solve(1.0)
    assert abs(e_planes[0] - e_rows[0]) <= 1e-12 * abs(e_rows[0]) and abs(e_planes[1] - e_rows[1]) <= 1e-12 * abs(e_rows[1])
    assert np.array_equal(la, b.get_labels()) and ra["energy"] == rb["energy"] and ra["rounds"] == rb["rounds"]
    a.close()
    b.close()


@pytest.mark.parametrize("tag,H,W,diagonal", [("diag", 11, 11, True), ("offdiag", 40, 50, False)])
def test_energy_parity_with_reference_gco_golden(tag, H, W, diagonal):
    """north_star: final MRF energy <= the reference's (gco alpha-beta swap through pygco's quantisation),
    on identical (logprob, graph, beta, init labels)."""
    g = np.load(os.path.join(G, "gco_%s.npz" % tag))
    K = int(g["K"])
    w, eid = R.edge_weights_from_distance(g["edges"], 0.5)
    n = g["logprob"].shape[0]
    b = _block(n, 4, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 8)
    b.set_logprob(g["logprob"])
    b.set_labels(g["init"])
    res = b.solve(float(g["beta"]))
    lab = b.get_labels()
    e_mine = R.mrf_energy(lab, g["logprob"], eid, w, float(g["beta"]))[0]
    np.testing.assert_allclose(res["energy"], e_mine, rtol=1e-6)
    e_ref = float(g["efloat_swap_pygco"][0])            # what the reference's E-step returns
    e_fine = float(g["efloat_swap_fine"][0])           # gco swap at its finest safe quantisation
    assert e_mine <= e_ref + 1e-6 * abs(e_ref), (e_mine, e_ref, e_fine)
    assert e_mine <= e_fine + 1e-6 * abs(e_fine), (e_mine, e_ref, e_fine)
    b.close()


# Sizes: the small ones from round 1, then BASELINE's own block sizes -- config 1's two blocks (652- and 683-bin diagonal
# blocks: 212,878 / 233,586 nodes, K=20) and config 2 in full (2000-bin diagonal block, 2,001,000 nodes, K=10).
LIVE_GCO_CASES = [(0, 150, 10, False, 0.0), (1, 160, 20, True, 0.0), (3, 120, 20, False, 0.3), (5, 220, 20, True, 0.15),
                  (7, 140, 30, False, 0.1), (11, 652, 20, True, 0.0), (12, 683, 20, True, 0.1), (13, 2000, 10, True, 0.0)]


@pytest.mark.parametrize("seed,N,K,diagonal,perturb", LIVE_GCO_CASES)
def test_energy_parity_with_live_gco_on_synthetic_blocks(seed, N, K, diagonal, perturb):
    """north_star: "final MRF energy <= the reference's", on seeded synthetic Hi-C blocks up to BASELINE's block sizes,
    gco run live (oracle/_ref travels with the repo), the solver at its exact fixed point (tol 0) and at the 1e-6
    relative stopping tolerance the fit driver and the bench use (tol 1000 ppb).

    The reference's result is gco's swap THROUGH PYGCO'S QUANTISATION (phylo_hmrf.py:496-498): the GPU labelling must
    be at or below it STRICTLY -- both labellings are scored by the same float64 function, no slack.  gco at its finest
    safe quantisation is not what the reference computes; the GPU labelling is required to be at or below it as well
    (neither local optimum dominates the other in theory -- global swap moves vs window-restricted expansion / fusion /
    chain moves at four scales -- but every case measured so far is below).  Measured (end of round 2, profiles/r2_y_live_gco_energy_gaps.txt): BELOW fine-quantised swap in every
    case, -1.0e-5 ... -3.5e-3, the 2,001,000-node K = 10 block from uniformly random labels included (-1.5e-5 at the
    stopping tolerance, -1.9e-5 at the exact fixed point)."""
    from oracle import gco_ref
    blk = synth.make_block(seed, N, N, 4, K, diagonal)
    X = blk["X"]
    n = X.shape[0]
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    means = blk["means"] + perturb * np.random.default_rng(seed + 1).standard_normal(blk["means"].shape)
    lp = R.log_multivariate_normal_density_full(X, means, blk["covars"])
    init = np.random.default_rng(seed + 7).integers(0, K, n)
    V = R.potts_matrix(K, 1.0)
    # The reference's energies: recorded in the build container by tests/golden/make_golden_live_gco.py (gco compiled from
    # /root/reference) and committed, so the assertion below holds on a box that never receives the research-licensed
    # binary; where the binary is present it is run live as well and must reproduce the recorded numbers.
    import json
    rec = [c for c in json.load(open(os.path.join(G, "live_gco_energies.json")))["cases"]
           if (c["seed"], c["N"], c["K"], c["diagonal"], c["perturb"]) == (seed, N, K, bool(diagonal), perturb)]
    assert len(rec) == 1, "no recorded gco energies for this case: run tests/golden/make_golden_live_gco.py"
    np.testing.assert_allclose(R.mrf_energy(init, lp, eid, w, 1.0)[0], rec[0]["e_init"], rtol=1e-12)    # same inputs
    e_ref = {"pygco": rec[0]["e_pygco"], "fine": rec[0]["e_fine"]}
    if gco_ref.available():
        for q in ("pygco", "fine"):
            lab = gco_ref.cut_general_graph(eid, w, -lp, V, n_iter=5000, algorithm="swap", init_labels=init, quant=q)
            np.testing.assert_allclose(R.mrf_energy(lab, lp, eid, w, 1.0)[0], e_ref[q], rtol=1e-12)
    b = _block(n, 4, K)
    b.set_graph(eid, w)
    b.set_grid(N, N, diagonal, 8)
    b.set_logprob(lp)
    for tol_ppb in (0, 1000, 10000):
        b.set_labels(init)
        res = b.solve(1.0, energy_tol_ppb=tol_ppb)
        e_mine = R.mrf_energy(b.get_labels(), lp, eid, w, 1.0)[0]
        print("n %d K %d tol %d ppb: energy GPU %.3f  swap via pygco %.3f (GPU %+.2e)  swap fine %.3f (GPU %+.2e)  rounds %d"
              % (n, K, tol_ppb, e_mine, e_ref["pygco"], (e_mine - e_ref["pygco"]) / abs(e_ref["pygco"]), e_ref["fine"],
                 (e_mine - e_ref["fine"]) / abs(e_ref["fine"]), res["rounds"]))
        assert res["converged"]
        assert e_mine <= e_ref["pygco"], (tol_ppb, e_mine, e_ref)
        # At the exact fixed point: strictly.  At the stopping tolerance the solve ends when a whole round gains less than
        # 1e-6 of |E|, i.e. a few 1e-6 short of its own fixed point: ten stopping tolerances are allowed against THIS
        # comparison (gco at a quantisation the reference does not use); measured: -3.5e-3 ... +1.9e-6 (the 2 M-node K = 10
        # cold start from random labels, 7 rounds).  The comparison with what the reference computes, above, has no allowance.
        assert e_mine <= e_ref["fine"] + 1e-8 * tol_ppb * abs(e_ref["fine"]), (tol_ppb, e_mine, e_ref)
    b.close()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_graph_expansion_is_the_exact_binary_optimum_on_small_graphs(seed):
    """maxflow.hip: one alpha-expansion of a general graph -- every node keeps its label or takes alpha -- is solved by a
    minimum cut (push-relabel on the device).  On random graphs of 14 nodes the result is compared with BRUTE FORCE over all
    2^(active nodes) switch sets, every labelling scored by the float64 oracle: the move's energy equals the optimum up to the
    quantisation of the capacities (the largest single term at 2^24; the allowance counts the nodes and arcs in which the
    move differs from the optimum: tests/maxflow_reference.expansion_allowance, where it is derived; larger graphs and the
    label-for-label comparison are in tests/test_gpu_maxflow.py), it never exceeds the energy before, and a second
    expansion of the same label changes nothing."""
    import itertools
    from tests.maxflow_reference import expansion_allowance
    rng = np.random.default_rng(100 + seed)
    n, K = 14, 4
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < 0.3]
    for i in range(n - 1):                                   # (connected, and no isolated node)
        if not any(i in pr for pr in pairs):
            pairs.append((i, i + 1))
    eid = np.array(sorted(set(pairs)), dtype=np.int64)
    w = rng.random(eid.shape[0]) * 1.5 + 0.05
    lp = -rng.random((n, K)) * 3.0
    labels = rng.integers(0, K, n)
    beta = 0.9
    b = _block(n, 4, K)
    b.set_graph(eid, w)
    b.set_logprob(lp)
    for alpha in range(K):
        b.set_labels(labels)
        e0 = R.mrf_energy(labels, lp, eid, w, beta)[0]
        active = np.flatnonzero(labels != alpha)
        best, best_set = e0, np.zeros(n, dtype=bool)
        for bits in itertools.product((0, 1), repeat=len(active)):
            cand = labels.copy()
            cand[active[np.flatnonzero(bits)]] = alpha
            e = R.mrf_energy(cand, lp, eid, w, beta)[0]
            if e < best:
                best, best_set = e, cand != labels
        ch = b.graph_expansion(beta, alpha)
        got = b.get_labels()
        assert ch == int(np.sum(got != labels)) and np.all((got == labels) | (got == alpha))
        e1 = R.mrf_energy(got, lp, eid, w, beta)[0]
        allow = expansion_allowance(n, eid, w, lp, labels, beta, alpha, got != labels, best_set)
        assert allow < n * max(np.abs(lp).max() * 2 + w.sum(), 1.0) / 2 ** 24          # (tighter than the bound it replaces)
        assert e1 <= e0 + 1e-9 and e1 <= best + allow, (alpha, e0, e1, best, allow)
        assert b.graph_expansion(beta, alpha) == 0
    b.close()


KNN_GCO_CASES = [(21, 50000, 10, 6, 0.0), (22, 30000, 20, 8, 0.1), (23, 8000, 6, 4, 0.2)]


@pytest.mark.parametrize("seed,n,K,k,perturb", KNN_GCO_CASES)
def test_energy_parity_with_gco_on_graphs_that_are_no_grid(seed, n, K, k, perturb):
    """The boundary is pygco.cut_general_graph on a GENERAL graph (phylo_hmrf.py:496-498, GCoptimization.h:551-597): the
    same energy bar OFF the contact-map stencil (which is all the reference itself ever builds, utility.py:1871-2053).
    There the solver has ICM, component moves, path moves (chain_kernel's exact all-K DP along induced paths) and -- the
    move that closes the gap -- every label's alpha-EXPANSION over the whole graph by an exact minimum cut on the device
    (maxflow.hip).  Seeded k-nearest-neighbour graphs of random points (oracle/synth.make_knn_block), uniformly random
    initial labels, gco's swap run in the build container under pygco's quantisation and the finest one
    (tests/golden/make_golden_knn_gco.py -> knn_gco_energies.json; reproduced live where oracle/_ref is present), both
    labellings scored by the same float64 function.  Asserted as on the grid: STRICTLY at or below what the reference
    computes, and at or below gco's finest quantisation (ten stopping tolerances allowed at the 1e-6 tolerance).  Measured:

      50,000 nodes / 176,382 edges / K = 10 / k = 6   GPU 227,569.3   gco via pygco 227,685.8 (-5.1e-4)   gco fine 227,589.8 (-9.0e-5)
      30,000 nodes / 138,459 edges / K = 20 / k = 8   GPU 118,948.3   gco via pygco 119,098.0 (-1.3e-3)   gco fine 118,962.2 (-1.2e-4)
       8,000 nodes /  19,428 edges / K =  6 / k = 4   GPU  36,251.7   gco via pygco  36,268.8 (-4.7e-4)   gco fine  36,257.9 (-1.7e-4)
      (ICM + components alone: +3.5e-4, -2.1e-4, +3.0e-3 against pygco; with the path moves: -3e-6, -9.4e-4, +1.25e-3)"""
    import json
    from oracle import gco_ref
    blk = synth.make_knn_block(seed, n, 4, K, k=k)
    X = blk["X"]
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    means = blk["means"] + perturb * np.random.default_rng(seed + 1).standard_normal(blk["means"].shape)
    lp = R.log_multivariate_normal_density_full(X, means, blk["covars"])
    init = np.random.default_rng(seed + 7).integers(0, K, n)
    V = R.potts_matrix(K, 1.0)
    rec = [c for c in json.load(open(os.path.join(G, "knn_gco_energies.json")))["cases"]
           if (c["seed"], c["n"], c["K"], c["k"], c["perturb"]) == (seed, n, K, k, perturb)]
    assert len(rec) == 1, "no recorded gco energies for this case: run tests/golden/make_golden_knn_gco.py"
    np.testing.assert_allclose(R.mrf_energy(init, lp, eid, w, 1.0)[0], rec[0]["e_init"], rtol=1e-12)    # same inputs
    e_ref = {"pygco": rec[0]["e_pygco"], "fine": rec[0]["e_fine"]}
    if gco_ref.available():
        for q in ("pygco", "fine"):
            lab = gco_ref.cut_general_graph(eid, w, -lp, V, n_iter=5000, algorithm="swap", init_labels=init, quant=q)
            np.testing.assert_allclose(R.mrf_energy(lab, lp, eid, w, 1.0)[0], e_ref[q], rtol=1e-12)
    b = _block(n, 4, K)
    b.set_graph(eid, w)
    b.set_logprob(lp)
    for tol_ppb in (0, 1000, 10000):
        b.set_labels(init)
        res = b.solve(1.0, energy_tol_ppb=tol_ppb)
        e_mine = R.mrf_energy(b.get_labels(), lp, eid, w, 1.0)[0]
        print("\nknn n %d K %d tol %d ppb: energy GPU %.3f  swap via pygco %.3f (GPU %+.2e)  swap fine %.3f (GPU %+.2e)  rounds %d"
              % (n, K, tol_ppb, e_mine, e_ref["pygco"], (e_mine - e_ref["pygco"]) / abs(e_ref["pygco"]), e_ref["fine"],
                 (e_mine - e_ref["fine"]) / abs(e_ref["fine"]), res["rounds"]))
        assert res["converged"]
        assert e_mine <= e_ref["pygco"], (tol_ppb, e_mine, e_ref)
        assert e_mine <= e_ref["fine"] + 1e-8 * tol_ppb * abs(e_ref["fine"]), (tol_ppb, e_mine, e_ref)
    b.close()


def test_energy_parity_chain_graph_without_geometry():
    g = np.load(os.path.join(G, "gco_chain.npz"))
    K = int(g["K"])
    w, eid = R.edge_weights_from_distance(g["edges"], 0.5)
    n = g["logprob"].shape[0]
    b = _block(n, 4, K)
    b.set_graph(eid, w)
    b.set_grid(1, n, False, 8)      # a 1 x n block: the chain is a grid row
    b.set_logprob(g["logprob"])
    b.set_labels(g["init"])
    res = b.solve(float(g["beta"]))
    e_ref = float(g["efloat_swap_fine"][0])
    # a single chain is solved EXACTLY by one row move: the global optimum, so <= any gco result
    assert res["energy"] <= e_ref + 1e-5 * abs(e_ref)
    b.close()


# ------------------------------------------------------------------------------------------------ b3
@pytest.mark.parametrize("et", [0, 3])
def test_posterior_stats_golden(et):
    g = np.load(os.path.join(G, "posteriors_et%d.npz" % et))
    X, labels, lp = g["X"], g["labels"], g["logprob"]
    n, K = lp.shape
    w, eid = R.edge_weights_from_distance(g["edges"], float(g["beta1"]))
    b = _block(n, X.shape[1], K)
    b.set_observations(X)
    b.set_graph(eid, w)
    b.set_logprob(lp)
    b.set_labels(labels)
    stats, costs, post = b.posterior_stats(float(g["beta"]), et, want_posteriors=True)
    assert np.max(np.abs(post - g["posteriors"])) < 2e-5
    np.testing.assert_allclose(stats["post"], g["post"], rtol=2e-5)
    np.testing.assert_allclose(stats["obs"], g["obs"], rtol=2e-5)
    np.testing.assert_allclose(stats["obs*obs.T"], g["obsobsT"], rtol=2e-5)
    ref = np.array([float(g["pairwise_cost"]), float(g["pairwise_cost_normalize"]), float(g["unary_cost"]), float(g["cost1"])])
    np.testing.assert_allclose(costs / n, ref, rtol=1e-5)
    b.close()


# (the last two: the kernel's corner -- K = 64, S = 8 takes 59.5 KB of LDS at 128-node tiles; K = 56 the size below, 52.7 KB)
@pytest.mark.parametrize("S,K,N", [(4, 20, 120), (8, 30, 60), (4, 10, 200), (8, 64, 50), (8, 56, 50)])
def test_posterior_stats_oracle(S, K, N):
    blk = synth.make_block(5, N, N, S, K, True)
    X = blk["X"]
    n = X.shape[0]
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    lp = R.log_multivariate_normal_density_full(X, blk["means"], blk["covars"])
    # keep the posterior numerically meaningful: soften the model so rows do not underflow in the reference formula
    lp = lp / max(1.0, np.abs(lp).max() / 200.0)
    rng = np.random.default_rng(1)
    labels = np.where(rng.random(n) < 0.8, np.argmax(lp, 1), rng.integers(0, K, n))
    V = R.potts_matrix(K, 1.0)
    post_ref, pc, pcn, uc, c1 = R.compute_posteriors_graph(labels, lp, eid, w, V, 3)
    st_ref = R.sufficient_statistics(post_ref, X)
    b = _block(n, S, K)
    b.set_observations(X)
    b.set_graph(eid, w)
    b.set_logprob(lp)
    b.set_labels(labels)
    stats, costs, post = b.posterior_stats(1.0, 3, want_posteriors=True)
    assert np.max(np.abs(post - post_ref)) < 2e-5
    for key in ("post", "obs", "obs*obs.T"):
        np.testing.assert_allclose(stats[key], st_ref[key], rtol=2e-5, atol=1e-6 * np.abs(st_ref[key]).max())
    np.testing.assert_allclose(costs / n, [pc, pcn, uc, c1], rtol=1e-5)
    # property: sum_k post[k] == n, and the trace identity sum_k obs*obs.T[k] == X^T X
    np.testing.assert_allclose(stats["post"].sum(), n, rtol=1e-6)
    np.testing.assert_allclose(stats["obs*obs.T"].sum(axis=0), X.T @ X, rtol=2e-5)
    # stats-only call (no posterior download) gives the same numbers
    stats2, costs2, none = b.posterior_stats(1.0, 3)
    assert none is None
    np.testing.assert_allclose(stats2["obs"], stats["obs"], rtol=1e-9)
    b.close()


# ------------------------------------------------------------------------------------------------ graph
@pytest.mark.parametrize("H,W,diagonal,nn", [(61, 61, True, 8), (40, 77, False, 8), (33, 33, True, 4), (1, 50, False, 8), (300, 5, False, 4)])
def test_device_graph_matches_reference_edge_builder(H, W, diagonal, nn):
    """phmrf_block_build_grid_graph vs the restated utility.py:1871-2053 edge builder + exp(-beta1 d)."""
    rng = np.random.default_rng(H * 7 + W)
    n = H * (H + 1) // 2 if diagonal else H * W
    X = np.abs(rng.standard_normal((n, 4))) + 0.01
    X[3] = 0.0                                   # a zero-norm node: the 1e-16 guard (utility.py:1939)
    e = R.grid_edges(X.astype(np.float32).astype(np.float64), H, W, diagonal, nn)
    w, eid = R.edge_weights_from_distance(e, 0.5)
    a = _block(n, 4, 3)
    a.set_observations(X)
    a.set_graph(eid, w)
    a.set_grid(H, W, diagonal, nn)
    nbr_a, wgt_a = a.get_adjacency()
    b = _block(n, 4, 3)
    b.set_observations(X)
    b.build_grid_graph(H, W, diagonal, nn, 0.5)
    nbr_b, wgt_b = b.get_adjacency()
    D = min(nbr_a.shape[1], nbr_b.shape[1])
    assert np.array_equal(nbr_a[:, :D], nbr_b[:, :D])
    assert np.all(nbr_a[:, D:] == -1) and np.all(nbr_b[:, D:] == -1)
    np.testing.assert_allclose(wgt_a[:, :D], wgt_b[:, :D], rtol=2e-6, atol=1e-7)
    # and the moves built on it behave identically on an exactly representable problem
    lp = -rng.integers(0, 9, (n, 3)).astype(np.float64)
    init = rng.integers(0, 3, n)
    for blk in (a, b):
        blk.set_logprob(lp)
        blk.set_labels(init)
    ra, rb = a.solve(1.0), b.solve(1.0)
    np.testing.assert_allclose(ra["energy"], rb["energy"], rtol=1e-5)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ api
def test_error_paths_and_label_slots():
    from phylo_hmrf_amd import PhmrfError
    b = _block(100, 4, 5)
    with pytest.raises(PhmrfError) as ei:
        b.solve(1.0)
    assert ei.value.status == 5            # graph not set
    edges = np.stack([np.arange(99), np.arange(1, 100)], 1)
    b.set_graph(edges, np.ones(99))
    with pytest.raises(PhmrfError):
        b.set_grid(7, 7, False, 8)         # 49 != 100
    with pytest.raises(PhmrfError):
        b.set_labels(np.full(100, 5))      # label out of range
    with pytest.raises(PhmrfError):
        b.set_graph(np.array([[0, 0]]), np.ones(1))   # self loop
    with pytest.raises(PhmrfError):
        b.set_graph(np.array([[0, 1], [1, 0]]), np.ones(2))   # duplicate
    b.set_graph(edges, np.ones(99))
    lab = np.arange(100) % 5
    b.set_labels(lab.astype(np.float64))   # float labels as the reference passes them (base.py:381,394)
    b.save_labels(1)
    b.set_labels(np.zeros(100))
    assert np.array_equal(b.get_saved_labels(1), lab)
    b.restore_labels(1)
    assert np.array_equal(b.get_labels(), lab)
    with pytest.raises(PhmrfError):
        b.restore_labels(2)
    b.close()


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_cfg2_properties():
    """BASELINE configs[1] at full size (2000 x 2000 diagonal block, 2,001,000 nodes, S=4, K=10) through
    size-independent properties: sampled emission rows vs the float64 oracle, sampled adjacency rows vs the restated
    edge builder, energy monotone under the solver and equal to the oracle's energy of the returned labels, statistics
    identities (sum_k post = n, sum_k obs*obs.T = X^T X, sum_k obs = sum_i x_i), idempotence of the converged solve."""
    import torch
    from phylo_hmrf_amd import Block, synthetic
    from phylo_hmrf_amd.tree import PhyloTree
    N, S, K = 2000, 4, 10
    n = N * (N + 1) // 2
    tree = PhyloTree(synthetic.tree_for(S))
    rng = np.random.default_rng(0)
    P = synthetic.sample_ou_params(rng, tree, K)
    mu, cv = tree.mean_cov(P)
    cv = cv + 1e-3 * np.eye(S)
    dev = torch.device("cuda", 0)
    Xd = synthetic.device_observations(torch, dev, 5, N, N, True, K, mu, cv)
    torch.cuda.synchronize()
    X = Xd.cpu().numpy().astype(np.float64)
    b = Block(n, S, K)
    b.set_observations_dev(Xd.data_ptr())
    b.sync()
    b.build_grid_graph(N, N, True, 8, 0.5)
    b.emission(mu, cv)
    lp = b.get_logprob()
    idx = rng.choice(n, 20000, replace=False)
    ref = R.log_multivariate_normal_density_full(X[idx], mu, cv)
    assert np.all(np.abs(lp[idx] - ref) <= _emission_tol(ref))
    # adjacency of sampled nodes: neighbours are exactly the valid 8-stencil cells, weights exp(-beta1 d)
    nbr, wgt = b.get_adjacency()
    ii, jj = np.triu_indices(N)
    start = np.concatenate([[0], np.cumsum(N - np.arange(N))])
    for v in rng.choice(n, 300, replace=False):
        i, j = ii[v], jj[v]
        exp_ids, exp_w = [], []
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                a, c = i + di, j + dj
                if (di or dj) and 0 <= a < N and 0 <= c < N and a <= c:
                    u = start[a] + (c - a)
                    d = ((X[v] - X[u]) ** 2).sum() / (np.linalg.norm(X[v]) * np.linalg.norm(X[u]) + 1e-16)
                    if i == j and a == c:
                        d *= 0.5
                    exp_ids.append(u)
                    exp_w.append(np.exp(-0.5 * d))
        got = nbr[v][nbr[v] >= 0]
        assert list(got) == sorted(exp_ids)
        order = np.argsort(exp_ids)
        np.testing.assert_allclose(wgt[v][:len(got)], np.array(exp_w)[order], rtol=2e-6, atol=1e-7)
    res = b.solve(1.0, init_mode=1)
    assert res["converged"] and res["energy"] < res["energy_init"]
    labels = b.get_labels()
    # oracle energy of the returned labels from the device adjacency (each undirected edge appears twice)
    e_un = -lp[np.arange(n), labels].sum()
    valid = nbr >= 0
    diff = valid & (labels[np.where(valid, nbr, 0)] != labels[:, None])
    e_pw = 0.5 * (wgt.astype(np.float64) * diff).sum()
    np.testing.assert_allclose(res["energy"], e_un + e_pw, rtol=1e-6)
    res2 = b.solve(1.0)
    assert res2["energy"] <= res["energy"] * (1 + 1e-9) and res2["rounds"] <= 2
    stats, costs, _ = b.posterior_stats(1.0, 3)
    np.testing.assert_allclose(stats["post"].sum(), n, rtol=1e-6)
    np.testing.assert_allclose(stats["obs"].sum(axis=0), X.sum(axis=0), rtol=2e-5)
    np.testing.assert_allclose(stats["obs*obs.T"].sum(axis=0), X.T @ X, rtol=2e-5)
    np.testing.assert_allclose(costs[2], e_un, rtol=1e-6)          # unary cost numerator = unary energy
    np.testing.assert_allclose(costs[0], 2.0 * e_pw, rtol=1e-5)    # pairwise cost counts every edge from both ends
    np.testing.assert_allclose(costs[3], costs[1] + costs[2], rtol=1e-12)
    b.close()


@pytest.mark.parametrize("H,W,K,diagonal,beta", [_as_before(48, 48, 6, True, 1.0), _as_before(20, 130, 4, False, 1.0),
                                                 (48, 48, 6, True, 0.5), (20, 130, 4, False, 2.0)])
def test_four_neighbour_grid_moves_and_solver(H, W, K, diagonal, beta):
    """num_neighbor = 4 (the reference's other stencil, utility.py:1917-1920): the grid-native strip inputs carry zero
    diagonal weights; strip passes equal the move model, every move is energy-non-increasing, the solver converges."""
    rng = np.random.default_rng(H + W)
    n = H * (H + 1) // 2 if diagonal else H * W
    X = rng.uniform(0.5, 2, (n, 2))
    e = R.grid_edges(X, H, W, diagonal, 4)
    eid = np.int64(e[:, :2])
    w = rng.integers(1, 9, len(eid)) / 8.0
    un = rng.integers(0, 12, (n, K)).astype(np.float64) * 0.5
    lp = -un
    init = rng.integers(0, K, n)
    g = M.Graph(n, eid, w)
    b = _block(n, 2, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 4)
    b.set_logprob(lp)
    b.set_labels(init)
    lab = init.astype(np.int64).copy()
    for orient, sr, sc, alpha in [(0, 0, 0, -1), (1, 2, 9, 1), (0, 4, 33, 0), (1, 1, 0, -1)]:
        prop = M.best_alternative(g, -lp, lab, beta) if alpha < 0 else np.full(n, alpha)
        ch_ref = M.strip_fusion(g, -lp, lab, prop, beta, H, W, diagonal, orient, sr, sc)
        ch = b.strip_pass(beta, orient, sr, sc, alpha)
        got = b.get_labels().astype(np.int64)
        assert np.array_equal(got, lab) and ch == ch_ref, (orient, alpha, int((got != lab).sum()))
    prev = b.energy(beta)[0]
    for fam in range(2):
        b.chain_sweep(beta, fam)
        en = b.energy(beta)[0]
        assert en <= prev + 1e-9
        prev = en
    res = b.solve(beta)
    assert res["converged"] and res["energy"] <= prev + 1e-9
    assert abs(res["energy"] - M.energy(g, -lp, b.get_labels().astype(np.int64), beta)[0]) < 1e-6
    b.close()


@pytest.mark.parametrize("H,W,diagonal,K,nn", [(1, 1, False, 3, 8), (2, 2, True, 2, 8), (3, 3, True, 1, 8), (1, 7, False, 4, 8),
                                              (7, 1, False, 4, 8), (5, 5, True, 64, 8), (12, 70, False, 64, 8),
                                              (6, 6, False, 40, 4), (64, 64, True, 2, 8), (65, 129, False, 3, 8)])
def test_degenerate_sizes(H, W, diagonal, K, nn):
    """A single node, one label, the maximum number of labels, one-row / one-column grids, strips narrower than a
    segment: the solver converges, never raises the energy, and reports the energy of the labels it returns."""
    rng = np.random.default_rng(H * 1000 + W + K)
    n = H * (H + 1) // 2 if diagonal else H * W
    X = rng.uniform(0.5, 2, (n, 2))
    e = R.grid_edges(X, H, W, diagonal, nn)
    eid = np.int64(e[:, :2]) if len(e) else np.zeros((0, 2), np.int64)
    w = rng.integers(1, 9, len(eid)) / 8.0
    b = _block(n, 2, K)
    b.set_observations(X)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, nn)
    lp = -rng.integers(0, 12, (n, K)).astype(np.float64) * 0.5
    b.set_logprob(lp)
    b.set_labels(rng.integers(0, K, n))
    e0 = b.energy(1.0)[0]
    res = b.solve(1.0)
    lab = b.get_labels().astype(np.int64)
    host = float((-lp)[np.arange(n), lab].sum())
    if len(eid):
        host = M.energy(M.Graph(n, eid, w), -lp, lab, 1.0)[0]
    assert res["converged"] and res["energy"] <= e0 + 1e-9
    assert abs(res["energy"] - host) <= 1e-6 * max(1.0, abs(host))
    b.close()


@pytest.mark.parametrize("N,S,K", [(4980, 4, 20), (24896, 4, 20), (4980, 8, 30)])
def test_full_size_largest_block_of_the_metric_config(N, S, K):
    """The largest block of the metric configuration (hg38 chr1 at 50 kb: 4980 x 4980 diagonal block, 12,402,690
    nodes, S=4, K=20), of BASELINE's config 5 (chr1 at 10 kb: 24896 x 24896, 309,917,856 nodes: the biggest single
    MRF the path holds on one GPU, 64-bit offsets everywhere) and of config 4 (the same 50 kb block with 8 species on
    the deeper tree and K=30) through properties that need no host copy of the big arrays: the solver lowers the energy and
    converges; the energy kernel, the solver's own report and the posterior kernel's cost numerators agree (three
    different kernels); statistics identities against torch reductions of X; a second solve changes (almost) nothing."""
    import torch
    from phylo_hmrf_amd import Block, synthetic
    from phylo_hmrf_amd.tree import PhyloTree
    n = N * (N + 1) // 2
    tree = PhyloTree(synthetic.tree_for(S))
    rng = np.random.default_rng(1)
    P = synthetic.sample_ou_params(rng, tree, K)
    mu, cv = tree.mean_cov(P)
    cv = cv + 1e-3 * np.eye(S)
    P2 = np.clip(P * (1 + 0.1 * rng.standard_normal(P.shape)), 1e-3, 50)      # fit with slightly wrong parameters
    mu2, cv2 = tree.mean_cov(P2)
    cv2 = cv2 + 1e-3 * np.eye(S)
    dev = torch.device("cuda", 0)
    Xd = synthetic.device_observations(torch, dev, 9, N, N, True, K, mu, cv)
    torch.cuda.synchronize()
    b = Block(n, S, K)
    b.set_observations_dev(Xd.data_ptr())
    b.sync()
    b.build_grid_graph(N, N, True, 8, 0.5)
    b.emission(mu2, cv2)
    res = b.solve(1.0, init_mode=1, energy_tol_ppb=1000)
    assert res["converged"] and res["energy"] < res["energy_init"] and res["rounds"] < 32
    e_tot, e_un, e_pw = b.energy(1.0)
    np.testing.assert_allclose(res["energy"], e_tot, rtol=1e-9)
    stats, costs, _ = b.posterior_stats(1.0, 3)
    np.testing.assert_allclose(costs[2], e_un, rtol=1e-6)          # unary cost numerator = unary energy
    np.testing.assert_allclose(costs[0], 2.0 * e_pw, rtol=1e-5)    # pairwise cost counts every edge from both ends
    np.testing.assert_allclose(costs[3], costs[1] + costs[2], rtol=1e-12)
    X64 = Xd.double()
    np.testing.assert_allclose(stats["post"].sum(), n, rtol=1e-6)
    np.testing.assert_allclose(stats["obs"].sum(axis=0), X64.sum(dim=0).cpu().numpy(), rtol=2e-5)
    np.testing.assert_allclose(stats["obs*obs.T"].sum(axis=0), (X64.T @ X64).cpu().numpy(), rtol=2e-5)
    labels = b.get_labels()
    assert labels.min() >= 0 and labels.max() < K and len(np.unique(labels)) > K // 2
    res2 = b.solve(1.0, energy_tol_ppb=1000)
    assert res2["energy"] <= res["energy"] * (1 + 1e-9)
    assert (res["energy"] - res2["energy"]) <= 1e-5 * abs(res["energy"])     # the first solve had reached the tolerance
    b.close()


DET_SCRIPT = r"""
import os, sys, hashlib
import numpy as np
sys.path.insert(0, os.environ["PHMRF_ROOT"])
import torch
from phylo_hmrf_amd import Block, synthetic
from phylo_hmrf_amd.tree import PhyloTree
K, S, N = 12, 4, 700
tree = PhyloTree(synthetic.tree_for(S)); rng = np.random.default_rng(4)
P = synthetic.sample_ou_params(rng, tree, K); mu, cv = tree.mean_cov(P); cv = cv + 1e-3 * np.eye(S)
P2 = np.clip(P * (1 + 0.15 * rng.standard_normal(P.shape)), 1e-3, 50); mu2, cv2 = tree.mean_cov(P2); cv2 = cv2 + 1e-3 * np.eye(S)
dev = torch.device("cuda", 0)
X = synthetic.device_observations(torch, dev, 2, N, N, True, K, mu, cv); torch.cuda.synchronize()
n = N * (N + 1) // 2
def stats_vec(b):
    st, costs, _ = b.posterior_stats(1.0, 3)
    return np.concatenate([np.ravel(v) for v in st.values()] + [costs])
out = []
for rep in range(3):
    b = Block(n, S, K); b.set_observations_dev(X.data_ptr()); b.sync(); b.build_grid_graph(N, N, True, 8, 0.5)
    b.emission(mu2, cv2)
    res = b.solve(1.0, energy_tol_ppb=1000, init_mode=1)           # a cold start: component moves, coarse moves, every kernel
    lab = b.get_labels()
    sv = stats_vec(b)
    assert np.array_equal(sv, stats_vec(b))
    out.append((hashlib.sha1(lab.tobytes()).hexdigest(), res["rounds"], repr(res["energy"]), hashlib.sha1(sv.tobytes()).hexdigest()))
    b.close()
os.environ["PHMRF_DETERMINISTIC"] = "0"                          # the default reduction (atomics) on the same labelling
b = Block(n, S, K); b.set_observations_dev(X.data_ptr()); b.sync(); b.build_grid_graph(N, N, True, 8, 0.5)
b.emission(mu2, cv2); b.set_labels(lab)
err = float(np.max(np.abs(stats_vec(b) - sv) / (1.0 + np.abs(sv))))
b.close()
print("RESULT", out)
print("ERR", err)
"""


def test_deterministic_mode_gives_identical_labellings():
    """PHMRF_DETERMINISTIC=1 (include/phmrf.h): three cold-start solves of the same 245,350-node block, each on a fresh
    block, return bit-identical labels, round counts, energies and posterior statistics.  (Without it the f32 atomics of the component move
    table make the labellings differ in a few nodes from run to run: not asserted, it is a matter of timing.)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PHMRF_ROOT=root, PHMRF_DETERMINISTIC="1")
    out = subprocess.run([sys.executable, "-c", DET_SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1]
    runs = eval(line[len("RESULT"):])
    assert len(runs) == 3 and runs[0] == runs[1] == runs[2], runs
    # the statistics and costs too (summed in workgroup order), equal to the default atomic sums up to rounding
    err = float([ln for ln in out.stdout.splitlines() if ln.startswith("ERR")][-1].split()[1])
    assert err < 1e-9, err


def test_coarse_labels_in_batches_give_the_one_by_one_sequence():
    """The coarse alpha-expansions build four labels' child problems per pass and rebuild a label's problem only after a move
    (decided on the device, solve.hip coarse_sweep_nocount).  The labellings must be those of the one-label-at-a-time order
    (PHMRF_COARSE_BATCH=1): with PHMRF_DETERMINISTIC=1 both runs of the cold-start script give the same label hash, round
    count and energy, bit for bit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    dev = os.path.join(root, "phylo_hmrf_amd", "libphmrf_dev.so")      # (the knob exists in the -DPHMRF_DEV build only)
    assert os.path.exists(dev), "libphmrf_dev.so not built (make -C phylo_hmrf_amd/csrc)"
    for batch in ("4", "1"):
        env = dict(os.environ, PHMRF_ROOT=root, PHMRF_DETERMINISTIC="1", PHMRF_COARSE_BATCH=batch)
        if batch != "4":
            env["PHMRF_LIB"] = dev                                     # the product library (batches of 4) against it
        out = subprocess.run([sys.executable, "-c", DET_SCRIPT.replace("range(3)", "range(1)")], capture_output=True, text=True,
                             timeout=600, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1]
        runs.append(eval(line[len("RESULT"):])[0])
    assert runs[0] == runs[1], runs
    assert runs[0][1] >= 3                       # (several rounds: the coarse scales did run)


def test_coarse_shortcuts_leave_the_labellings_alone():
    """Round 4: a label's problem is rebuilt only in the wavefronts whose nodes carry a change stamp later than the batch's
    pass (coarsen_kernel; PHMRF_COARSE_NO_STAMP_GATE=1: everywhere), and a child strip is staged only if it holds a
    super-cell that proposes a switch -- while nothing has switched yet: a NEGATIVE switch cost that the one-hop flow
    certificate cannot settle (strip_kernel, debug & 32; PHMRF_NO_PIN_LOOK=1: every strip is staged and walked).  Both are
    exact: with PHMRF_DETERMINISTIC=1 the cold-start script
    gives the same label hash, round count and energy with and without them, bit for bit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    dev = os.path.join(root, "phylo_hmrf_amd", "libphmrf_dev.so")      # (the knobs exist in the -DPHMRF_DEV build only)
    assert os.path.exists(dev), "libphmrf_dev.so not built (make -C phylo_hmrf_amd/csrc)"
    for extra in ({}, {"PHMRF_COARSE_NO_STAMP_GATE": "1", "PHMRF_LIB": dev}, {"PHMRF_NO_PIN_LOOK": "1", "PHMRF_LIB": dev}):
        env = dict(os.environ, PHMRF_ROOT=root, PHMRF_DETERMINISTIC="1", **extra)
        out = subprocess.run([sys.executable, "-c", DET_SCRIPT.replace("range(3)", "range(1)")], capture_output=True, text=True,
                             timeout=600, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1]
        runs.append(eval(line[len("RESULT"):])[0])
    assert runs[0] == runs[1] == runs[2], runs
    assert runs[0][1] >= 3


GROUP_SCRIPT = r"""
import os, sys, hashlib
import numpy as np
sys.path.insert(0, os.environ["PHMRF_ROOT"])
import torch
from phylo_hmrf_amd import Block, synthetic
from phylo_hmrf_amd.tree import PhyloTree
K, S = 12, 4
tree = PhyloTree(synthetic.tree_for(S)); rng = np.random.default_rng(4)
P = synthetic.sample_ou_params(rng, tree, K); mu, cv = tree.mean_cov(P); cv = cv + 1e-3 * np.eye(S)
P2 = np.clip(P * (1 + 0.15 * rng.standard_normal(P.shape)), 1e-3, 50); mu2, cv2 = tree.mean_cov(P2); cv2 = cv2 + 1e-3 * np.eye(S)
P3 = np.clip(P2 * (1 + 0.05 * rng.standard_normal(P.shape)), 1e-3, 50); mu3, cv3 = tree.mean_cov(P3); cv3 = cv3 + 1e-3 * np.eye(S)
dev = torch.device("cuda", 0)
shapes = [(500, 500, True), (300, 420, False), (260, 260, True)]
opts = dict(energy_tol_ppb=1000)
out = []
for mode in ("one by one", "group"):
    blocks = []                          # (fresh blocks per mode: a block's solves cycle through the three strip cuts)
    for i, (H, W, diag) in enumerate(shapes):
        X = synthetic.device_observations(torch, dev, 10 + i, H, W, diag, K, mu, cv); torch.cuda.synchronize()
        n = H * (H + 1) // 2 if diag else H * W
        b = Block(n, S, K); b.set_observations_dev(X.data_ptr()); b.sync(); b.build_grid_graph(H, W, diag, 8, 0.5)
        blocks.append(b)
    for b in blocks:
        b.emission(mu2, cv2)
    if mode == "group":
        Block.solve_group(blocks, 1.0, init_mode=1, **opts)                  # cold
    else:
        for b in blocks: b.solve_fast(1.0, init_mode=1, **opts)
    for b in blocks:
        b.emission(mu3, cv3)
    if mode == "group":
        Block.solve_group(blocks, 1.0, **opts)                               # warm
    else:
        for b in blocks: b.solve_fast(1.0, **opts)
    out.append([hashlib.sha1(b.get_labels().tobytes()).hexdigest() for b in blocks])
    for b in blocks:
        b.close()
print("RESULT", out)
"""


def test_group_solve_in_lockstep_rounds_gives_the_per_block_labellings():
    """phmrf_mrf_solve_group (round 6): three independent blocks -- two triangular, one rectangular -- solved in lockstep rounds
    from one host thread, cold and then warm, give block for block the labels of solving them one after the other
    (PHMRF_DETERMINISTIC=1: bit for bit): the group call only interleaves the blocks' own state machines."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PHMRF_ROOT=root, PHMRF_DETERMINISTIC="1")
    out = subprocess.run([sys.executable, "-c", GROUP_SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1]
    runs = eval(line[len("RESULT"):])
    assert runs[0] == runs[1] and len(set(runs[0])) == 3, runs


PREP_SCRIPT = r"""
import os, sys, hashlib
import numpy as np
sys.path.insert(0, os.environ["PHMRF_ROOT"])
import torch
from phylo_hmrf_amd import Block, synthetic
from phylo_hmrf_amd.tree import PhyloTree
K, S, N = 12, 4, 500
mode = os.environ["PREP_MODE"]
tree = PhyloTree(synthetic.tree_for(S)); rng = np.random.default_rng(4)
P = synthetic.sample_ou_params(rng, tree, K); mu, cv = tree.mean_cov(P); cv = cv + 1e-3 * np.eye(S)
P2 = np.clip(P * (1 + 0.15 * rng.standard_normal(P.shape)), 1e-3, 50); mu2, cv2 = tree.mean_cov(P2); cv2 = cv2 + 1e-3 * np.eye(S)
P3 = np.clip(P2 * (1 + 0.05 * rng.standard_normal(P.shape)), 1e-3, 50); mu3, cv3 = tree.mean_cov(P3); cv3 = cv3 + 1e-3 * np.eye(S)
dev = torch.device("cuda", 0)
X = synthetic.device_observations(torch, dev, 2, N, N, True, K, mu, cv); torch.cuda.synchronize()
n = N * (N + 1) // 2
b = Block(n, S, K); b.set_observations_dev(X.data_ptr()); b.sync(); b.build_grid_graph(N, N, True, 8, 0.5)
b.emission(mu2, cv2)
b.solve(1.0, energy_tol_ppb=1000, init_mode=1)
b.save_labels(1)
out = []
# a warm E-step as the EM driver runs it, with the hint (a) not given, (b) given, (c) given and the labels changed behind it
if mode in ("hint", "hint_then_other_labels"):
    b.prepare_components()
if mode == "hint_then_other_labels":
    lab = b.get_labels().copy(); lab[: n // 3] = (lab[: n // 3] + 1) % K
    b.set_labels(lab)
if mode == "other_labels":
    lab = b.get_labels().copy(); lab[: n // 3] = (lab[: n // 3] + 1) % K
    b.set_labels(lab)
b.emission(mu3, cv3)
res = b.solve(1.0, energy_tol_ppb=1000)
out.append((hashlib.sha1(b.get_labels().tobytes()).hexdigest(), res["rounds"], repr(res["energy"])))
# ... and a second warm E-step after it (the hint is used once: this one computes its own components)
b.emission(mu2, cv2)
res = b.solve(1.0, energy_tol_ppb=1000)
out.append((hashlib.sha1(b.get_labels().tobytes()).hexdigest(), res["rounds"], repr(res["energy"])))
print("RESULT", out)
"""


def test_prepared_components_change_nothing_but_the_time():
    """phmrf_block_prepare_components (ABI 121) queues the connected components of the block's labels ahead of the solve
    that uses them (the EM driver: behind the host's M-step, /root/reference/base.py:399 is where the reference's M-step
    sits).  The next component pass compares, on the device, the labels it finds with the labels prepared for and
    recomputes when they differ.  With PHMRF_DETERMINISTIC=1: a warm E-step gives the same labels, rounds and energy with
    and without the hint; with the labels replaced between the hint and the solve it gives what the same replacement
    gives without the hint."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for mode in ("plain", "hint", "other_labels", "hint_then_other_labels"):
        env = dict(os.environ, PHMRF_ROOT=root, PHMRF_DETERMINISTIC="1", PREP_MODE=mode)
        out = subprocess.run([sys.executable, "-c", PREP_SCRIPT], capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        res[mode] = eval([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1][len("RESULT"):])
    assert res["plain"] == res["hint"], res
    assert res["other_labels"] == res["hint_then_other_labels"], res
    assert res["plain"] != res["other_labels"]            # (the replacement is not a no-op)


def test_xcd_aware_order_of_the_strips_leaves_the_labellings_alone():
    """Round 5: in orientation 1 the workgroups of strip_cols_kernel / fusion_cols_kernel take the strips in an XCD-aware
    order (groups of six adjacent bands dealt round-robin to the eight XCD labels, strip_of_slot in strip.hip) instead of the
    strips' own -- a bijection onto the strips plus padding workgroups, and the strips of a launch are independent, so the
    labelling cannot depend on it.  PHMRF_NO_XCD_MAP=1 (development library) runs them in their own order: with
    PHMRF_DETERMINISTIC=1 the cold-start script (700 x 700 upper triangle: 117 bands = 20 groups, three rounds of the eight
    labels with four padding groups) gives the same label hash, round count and energy either way, bit for bit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dev = os.path.join(root, "phylo_hmrf_amd", "libphmrf_dev.so")
    assert os.path.exists(dev), "libphmrf_dev.so not built (make -C phylo_hmrf_amd/csrc)"
    runs = []
    for extra in ({}, {"PHMRF_LIB": dev}, {"PHMRF_NO_XCD_MAP": "1", "PHMRF_LIB": dev}):
        env = dict(os.environ, PHMRF_ROOT=root, PHMRF_DETERMINISTIC="1", **extra)
        out = subprocess.run([sys.executable, "-c", DET_SCRIPT.replace("range(3)", "range(1)")], capture_output=True, text=True,
                             timeout=600, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1]
        runs.append(eval(line[len("RESULT"):])[0])
    assert runs[0] == runs[1] == runs[2], runs
    assert runs[0][1] >= 3


@pytest.mark.parametrize("H,W,diagonal", [(520, 610, False), (800, 800, True)])
def test_energy_of_later_rounds_from_the_touched_nodes_equals_the_full_pass(H, W, diagonal):
    """From its second round on a solve of a large grid block adds the CHANGE of the energy on the nodes the round's moves
    stamped to the previous evaluation (energy_delta_grid_kernel) instead of passing over the block again.  The energies it
    reports -- cold start with many rounds, warm start, exact convergence and tolerance stop -- must be those of the full
    pass (phmrf_mrf_energy), on a rectangular (off-diagonal) and on an upper-triangular block."""
    import torch
    from phylo_hmrf_amd import Block, synthetic
    from phylo_hmrf_amd.tree import PhyloTree
    S, K = 4, 12
    n = H * (H + 1) // 2 if diagonal else H * W
    assert n >= 1 << 18                                    # (smaller blocks always take the full pass)
    tree = PhyloTree(synthetic.tree_for(S))
    rng = np.random.default_rng(3)
    P = synthetic.sample_ou_params(rng, tree, K)
    mu, cv = tree.mean_cov(P)
    cv = cv + 1e-3 * np.eye(S)
    dev = torch.device("cuda", 0)
    Xd = synthetic.device_observations(torch, dev, 4, H, W, diagonal, K, mu, cv)
    torch.cuda.synchronize()
    b = Block(n, S, K)
    b.set_observations_dev(Xd.data_ptr())
    b.sync()
    b.build_grid_graph(H, W, diagonal, 8, 0.5)
    P2 = np.clip(P * (1 + 0.1 * rng.standard_normal(P.shape)), 1e-3, 50)
    mu2, cv2 = tree.mean_cov(P2)
    b.emission(mu2, cv2 + 1e-3 * np.eye(S))
    for kw in (dict(init_mode=1, energy_tol_ppb=1000), dict(energy_tol_ppb=0)):
        res = b.solve(1.0, **kw)
        assert res["rounds"] >= 2
        e_tot, e_un, e_pw = b.energy(1.0)
        np.testing.assert_allclose([res["energy"], res["energy_unary"], res["energy_pair"]], [e_tot, e_un, e_pw], rtol=1e-11)
    P3 = np.clip(P2 * (1 + 0.03 * rng.standard_normal(P.shape)), 1e-3, 50)                 # the next EM iteration's warm start
    mu3, cv3 = tree.mean_cov(P3)
    b.emission(mu3, cv3 + 1e-3 * np.eye(S))
    res = b.solve(1.0, energy_tol_ppb=1000)
    e_tot, e_un, e_pw = b.energy(1.0)
    assert res["rounds"] >= 2 and res["energy"] < res["energy_init"]
    np.testing.assert_allclose([res["energy"], res["energy_unary"], res["energy_pair"]], [e_tot, e_un, e_pw], rtol=1e-11)
    b.close()


def test_warm_start_choice_from_the_difference_equals_the_choice_from_two_energies():
    """phmrf_block_warm_start without a report (the fit's and the bench's call): on a large grid block the choice between the
    current labels and the snapshot comes from E(current) - E(snapshot) summed over the nodes where the two differ
    (energy_diff_grid_kernel) instead of from two full energy passes.  Same decision as the reported energies give, in both
    directions, on an upper-triangular and on a rectangular block; the difference itself is checked against the float64
    oracle through the reported energies (rel 1e-6 each)."""
    import torch
    from phylo_hmrf_amd import Block, synthetic
    from phylo_hmrf_amd.tree import PhyloTree
    K, S = 8, 4
    tree = PhyloTree(synthetic.tree_for(S))
    rng = np.random.default_rng(12)
    P = synthetic.sample_ou_params(rng, tree, K)
    mu, cv = tree.mean_cov(P)
    cv = cv + 1e-3 * np.eye(S)
    dev = torch.device("cuda", 0)
    for H, W, diag in ((420, 420, True), (260, 300, False)):
        X = synthetic.device_observations(torch, dev, 3, H, W, diag, K, mu, cv)
        torch.cuda.synchronize()
        n = X.shape[0]
        assert n >= 1 << 16
        b = Block(n, S, K)
        b.set_observations_dev(X.data_ptr())
        b.sync()
        b.build_grid_graph(H, W, diag, 8, 0.5)
        b.emission(mu, cv)
        b.solve_fast(1.0, init_mode=1, energy_tol_ppb=1000)
        good = b.get_labels()
        worse = good.copy()
        idx = rng.choice(n, size=n // 40, replace=False)
        worse[idx] = rng.integers(0, K, idx.size)
        for cur, snap in ((good, worse), (worse, good), (good, good)):
            b.set_labels(snap)
            b.save_labels(1)
            b.set_labels(cur)
            ec, es, took = b.warm_start(1.0, 1, choose=False)                # the two energies, nothing chosen
            assert np.array_equal(b.get_labels(), cur)
            b.warm_start(1.0, 1, report=False)                                # the choice, from the difference
            chosen = b.get_labels()
            want = snap if not (ec < es) else cur
            assert np.array_equal(chosen, want), (diag, ec, es)
            assert took == (not (ec < es))
        b.close()
