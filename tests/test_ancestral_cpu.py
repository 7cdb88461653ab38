"""CPU: the host side of the ancestral reconstruction -- the joint Gaussian of all tree nodes and the conditioning tables
(phylo_hmrf_amd/tree.py) against mean_cov, plain conditioning and a simulation of the recursion; the float64 reference of
the kernel (tests/ancestral_reference.py) on tables whose answer is known; the command line's refusals and the .npz."""
import numpy as np
import pytest

from phylo_hmrf_amd import synthetic
from phylo_hmrf_amd.tree import PhyloTree
from tests import ancestral_reference as AR

EXAMPLE_TREE = [[0, 1], [1, 2], [1, 3], [3, 4], [4, 5], [4, 6], [3, 7]]      # N = 8, leaves 2 5 6 7, the root has one child
MIN_COVAR = 2e-3
AR_WEIGHTINGS = ("posterior", "called")
TREES = [("example", EXAMPLE_TREE)] + [("S%d" % S, synthetic.tree_for(S)) for S in range(2, 9)]


def _params(tree, K, seed):
    """random OU parameters in the fit's box; state 0 has one branch at beta = 0 (e = 1, no noise on that branch)"""
    rng = np.random.default_rng(seed)
    P = synthetic.sample_ou_params(rng, tree, K)
    P[0, 1 + int(rng.integers(0, tree.branch_dim))] = 0.0
    return P


@pytest.fixture(scope="module", params=TREES, ids=[t[0] for t in TREES])
def case(request):
    tree = PhyloTree(request.param[1])
    return tree, _params(tree, 3, 7 + tree.node_num)


def test_example_tree_is_the_synthetic_four_leaf_tree():
    tree = PhyloTree(EXAMPLE_TREE)
    assert synthetic.tree_for(4) == EXAMPLE_TREE
    assert (tree.node_num, tree.n_leaves) == (8, 4)
    assert tree.internal_nodes.tolist() == [0, 1, 3, 4] and tree.leaf_vec.tolist() == [2, 5, 6, 7]


def test_joint_moments_leaf_block_is_mean_cov(case):
    tree, P = case
    mean, cov = tree.joint_moments(P)
    means, covars = tree.mean_cov(P, MIN_COVAR)
    L = tree.leaf_vec
    assert mean.shape == (3, tree.node_num) and cov.shape == (3, tree.node_num, tree.node_num)
    np.testing.assert_allclose(mean[:, L], means, rtol=0, atol=1e-12)
    np.testing.assert_allclose(cov[:, L[:, None], L[None, :]], covars - MIN_COVAR * np.eye(tree.n_features), rtol=0, atol=1e-12)
    assert sorted(tree.internal_nodes.tolist() + L.tolist()) == list(range(tree.node_num))


def test_joint_moments_is_a_covariance(case):
    tree, P = case
    _, cov = tree.joint_moments(P)
    _, var, _, _ = tree.node_moments(P)
    for k in range(len(P)):
        assert np.array_equal(cov[k], cov[k].T)
        assert np.array_equal(np.diag(cov[k]), var[k])
        assert np.linalg.eigvalsh(cov[k]).min() >= -1e-12 * np.trace(cov[k])


def test_joint_moments_obeys_the_recursion(case):
    """Cov(X_i, X_j) = e_i Cov(X_parent(i), X_j) for every j that is no descendant of i: the recursion itself"""
    tree, P = case
    _, cov = tree.joint_moments(P)
    _, _, e, _ = tree.node_moments(P)
    for i in tree.order:
        below = [j for j in range(tree.node_num) if tree.node_anc[i, j] == i]
        others = [j for j in range(tree.node_num) if j not in below]
        np.testing.assert_allclose(cov[:, i, others], e[:, i, None] * cov[:, tree.parent[i], others], rtol=1e-12, atol=1e-15)


def test_tables_solve_the_normal_equations(case):
    tree, P = case
    affine, cond_var = tree.ancestral_tables(P, MIN_COVAR)
    mean, cov = tree.joint_moments(P)
    A, L = tree.internal_nodes, tree.leaf_vec
    S = tree.n_features
    assert affine.shape == (3, len(A), S + 1) and cond_var.shape == (3, len(A))
    assert np.all(cond_var >= 0)
    for k in range(3):
        G, c = affine[k, :, 1:], affine[k, :, 0]
        C_AL = cov[k][A[:, None], L[None, :]]
        lhs = G @ (cov[k][L[:, None], L[None, :]] + MIN_COVAR * np.eye(S))
        assert np.max(np.abs(lhs - C_AL)) <= 1e-10 * np.max(np.abs(C_AL))
        np.testing.assert_allclose(c + G @ mean[k, L], mean[k, A], rtol=1e-12, atol=1e-12)
        assert np.all(cond_var[k] <= cov[k][A, A] + 1e-12)                   # conditioning never adds variance


def test_reference_at_one_state_is_plain_conditioning(case):
    """K = 1: both weightings are the Gaussian conditional of the internal nodes given the noisy leaves, computed here from
    the joint covariance of [A | L] by the Schur complement"""
    tree, P = case
    P1 = P[:1]
    affine, cond_var = tree.ancestral_tables(P1, MIN_COVAR)
    mean, cov = tree.joint_moments(P1)
    A, L = tree.internal_nodes, tree.leaf_vec
    S = tree.n_features
    rng = np.random.default_rng(3)
    X = rng.normal(1.0, 1.0, (50, S))
    C_LL = cov[0][L[:, None], L[None, :]] + MIN_COVAR * np.eye(S)
    C_AL = cov[0][A[:, None], L[None, :]]
    inv = np.linalg.inv(C_LL)
    want_mean = mean[0, A][:, None] + C_AL @ inv @ (X - mean[0, L]).T
    want_var = np.diag(cov[0][A[:, None], A[None, :]] - C_AL @ inv @ C_AL.T)
    for weighting in ("posterior", "called"):
        m, v = AR.reconstruct(np.ones((50, 1)), np.zeros(50, dtype=np.int64), X, affine, cond_var, weighting)
        np.testing.assert_allclose(m, want_mean, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(v, np.repeat(np.maximum(want_var, 0.0)[:, None], 50, axis=1), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name,edges", [TREES[0], TREES[4], TREES[7]], ids=["example", "S5", "S8"])
def test_simulated_recursion_confirms_the_tables(name, edges):
    """250,000 draws of all nodes of one state, the leaves observed with noise min_covar: the residual z_A - (c + G x) has
    mean 0 within 5 standard errors, 5 sqrt(v / n), and variance cond_var within 5 v sqrt(2 / n), for every internal node"""
    tree = PhyloTree(edges)
    P = _params(tree, 1, 11)[0]                                                # (one of its branches at beta = 0)
    n = 250000
    rng = np.random.default_rng(5)
    Z = AR.simulate(tree, P, n, rng)
    X = Z[:, tree.leaf_vec] + np.sqrt(MIN_COVAR) * rng.standard_normal((n, tree.n_features))
    affine, cond_var = tree.ancestral_tables(P[None], MIN_COVAR)
    pred, v = AR.reconstruct(np.ones((n, 1)), np.zeros(n, dtype=np.int64), X, affine, cond_var, "called")
    res = Z[:, tree.internal_nodes].T - pred
    for a in range(len(tree.internal_nodes)):
        va = cond_var[0, a]
        assert np.array_equal(v[a], np.full(n, va))
        assert abs(res[a].mean()) <= 5 * np.sqrt(va / n), (a, res[a].mean(), va)
        assert abs(res[a].var() - va) <= 5 * va * np.sqrt(2.0 / n), (a, res[a].var(), va)


def test_reference_with_identity_tables_returns_the_posteriors():
    rng = np.random.default_rng(1)
    n, K, S = 40, 5, 3
    post = rng.dirichlet(np.ones(K), n)
    labels = rng.integers(0, K, n)
    affine = np.zeros((K, K, S + 1))
    affine[np.arange(K), np.arange(K), 0] = 1.0
    X = rng.normal(size=(n, S))
    mean, var = AR.reconstruct(post, labels, X, affine, np.zeros((K, K)), "posterior")
    assert np.array_equal(mean, post.T)
    np.testing.assert_allclose(var, (post * (1.0 - post)).T, rtol=1e-12, atol=1e-15)      # a Bernoulli's variance
    mean, var = AR.reconstruct(post, labels, X, affine, np.zeros((K, K)), "called")
    assert np.array_equal(mean, np.eye(K)[labels].T) and not var.any()


def test_reference_bounds_are_positive_and_small():
    rng = np.random.default_rng(2)
    n, K, S, A = 30, 4, 3, 2
    post = rng.dirichlet(np.ones(K), n)
    affine = rng.uniform(-2, 2, (K, A, S + 1))
    cv = rng.uniform(0, 1, (K, A))
    X = rng.uniform(0, 4, (n, S))
    for weighting in AR_WEIGHTINGS:
        bm, bv = AR.bounds(post, rng.integers(0, K, n), X, affine, cv, weighting)
        assert bm.shape == bv.shape == (A, n) and np.all(bm > 0) and np.all(bv >= 0) and bm.max() < 1e-2 and bv.max() < 1e-1


# ---- the command line ------------------------------------------------------------------------------------------------------
def _cli(**extra):
    import phylo_hmrf as cli
    return cli.run("4", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", "unused_output", synthetic="48",
                   seed="1", quiet="1", **extra)


@pytest.mark.parametrize("extra,names", [(dict(ancestral="posterior"), "--segment"),
                                         (dict(ancestral="called", postprocess="some.mat"), "--postprocess"),
                                         (dict(ancestral="both", segment="m.npz"), "--segment")])
def test_cli_refuses_ancestral_without_its_segmentation(extra, names, tmp_path, monkeypatch):
    """alone, with --postprocess, with another value: refused before any file is read or written, naming the other flag"""
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        _cli(**extra)
    assert "--ancestral" in str(e.value) and names in str(e.value)
    assert not list(tmp_path.iterdir())


def test_cli_parser_knows_the_option(monkeypatch):
    import phylo_hmrf as cli
    monkeypatch.setattr("sys.argv", ["phylo_hmrf.py", "--segment", "m.npz", "--ancestral", "called"])
    assert cli.parse_args().ancestral == "called"
    monkeypatch.setattr("sys.argv", ["phylo_hmrf.py"])
    assert cli.parse_args().ancestral == ""


def test_npz_round_trip(tmp_path):
    from phylo_hmrf_amd import ancestral
    tree = PhyloTree(EXAMPLE_TREE)
    rng = np.random.default_rng(4)
    res = dict(nodes=tree.internal_nodes, parent=tree.parent, mean=rng.normal(size=(4, 11)).astype(np.float32),
               sd=rng.random((4, 11)).astype(np.float32))
    lv = [[11, 0, 11, 4, 4, 0, 0, 0, 1, 1]]
    path = ancestral.save_npz(str(tmp_path / "a.npz"), res, "posterior", lv, species=["hg38", "panTro5", "gorGor4", "calJac3"])
    with np.load(path, allow_pickle=False) as z:                              # (no pickles: loads with them refused)
        assert sorted(z.files) == sorted(ancestral.NPZ_KEYS)
    d = ancestral.load_npz(path)
    assert d["weighting"] == "posterior" and d["species"] == ["hg38", "panTro5", "gorGor4", "calJac3"]
    assert d["nodes"].tolist() == [0, 1, 3, 4] and d["parent"].tolist() == tree.parent.tolist()
    assert np.array_equal(d["mean"], res["mean"]) and np.array_equal(d["sd"], res["sd"]) and d["len_vec"].tolist() == lv
    d = ancestral.load_npz(ancestral.save_npz(str(tmp_path / "b.npz"), dict(res, sd=None), "called", lv))
    assert d["sd"] is None and d["species"] == [] and d["weighting"] == "called" and np.array_equal(d["mean"], res["mean"])
