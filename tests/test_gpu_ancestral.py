"""GPU: the ancestral reconstruction -- ancestral_kernel (phmrf_ancestral) in every compiled form against the float64
reference (tests/ancestral_reference.py) within per-element float32 bounds, its posteriors against posterior_kernel's bit
for bit, the second trip of its grid-stride loop, row tiles, determinism, the status codes, and phyloHMRF.ancestral() end
to end: on simulated ancestors, through the command line, and on two ranks.

The bounds (ancestral_reference.bounds, derived there) are per element, from u = 2^-24 and the pinned 2e-5 of the device's
posteriors; every case prints its largest error / bound."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref_numpy as R
from oracle import synth
from tests import ancestral_reference as AR
from tests import posterior_reference as P
from tests.posterior_cases import MODES, _case, _f32, _nodes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTINGS = ("posterior", "called")
ANC_GRID_CAP = 2048                   # launch_ancestral_s: at most 2048 workgroups of 256 rows (K <= 40)
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = 0, 1, 4, 5


def _tile_threads(K):
    return 256 if K <= 40 else 128


def _tables(rng, K, A, S):
    """random maps with |c|, |G| <= 2 and variances in [0, 1], rounded to float32 before anybody sees them"""
    return _f32(rng.uniform(-2.0, 2.0, (K, A, S + 1))), _f32(rng.uniform(0.0, 1.0, (K, A)))


def _ratio(err, bound):
    """largest err / bound; an element with a bound of 0 must be exact"""
    assert np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def _compare(tag, mean, sd, post, labels, X, affine, cv, weighting):
    """the planes against the float64 reference, per element, within ancestral_reference.bounds"""
    assert mean.dtype == np.float32 and sd.dtype == np.float32 and mean.shape == sd.shape == (affine.shape[1], len(labels))
    ref_m, ref_v = AR.reconstruct(post, labels, X, affine, cv, weighting)
    bm, bv = AR.bounds(post, labels, X, affine, cv, weighting)
    rm = _ratio(np.abs(mean.astype(np.float64) - ref_m), bm)
    rv = _ratio(np.abs(sd.astype(np.float64) ** 2 - ref_v), bv)
    print("%s %s: mean err / bound %.3f, sd^2 err / bound %.3f" % (tag, weighting, rm, rv))
    assert rm <= 1.0 and rv <= 1.0, (tag, weighting, rm, rv)
    assert np.all(sd >= 0)
    return rm, rv


def _check_case(c, A, seed):
    affine, cv = _tables(np.random.default_rng(seed), c.K, A, c.S)
    b = c.block()
    tag = "n=%d K=%d S=%d A=%d et=%d %s" % (c.n, c.K, c.S, A, c.et, c.form)
    for weighting in WEIGHTINGS:
        mean, sd = b.ancestral(c.beta, c.et, affine, cv, weighting)
        _compare(tag, mean, sd, c.post, c.labels, c.X, affine, cv, weighting)
    b.close()


# ---- (a) the form and size matrix ------------------------------------------------------------------------------------
FORMS = ("grid_diag", "grid_rect", "explicit8", "ragged4", "isolated")
N_SPECS = ("1", "65", "TB-1", "TB+1", "2TB+1")
KS, SS, AS, ETS, BETAS = (1, 2, 7, 20, 33, 64), (1, 3, 4, 8), (1, 3, 4, 7, 16), (0, 3), (0.3, 1.3)


def _matrix():
    """30 cases that cycle through the forms, sizes, K, S, A and estimate_type (every value of each several times, every
    form at every size class it admits) instead of crossing them, and the corner K = 64, S = 8, A = 16 at n = 129"""
    cases = []
    for i in range(30):
        form, K, S = FORMS[i % 5], KS[i % 6], SS[i % 4]
        TB = _tile_threads(K)
        j = i + i // 5
        while _nodes(N_SPECS[j % 5], form, TB) is None:          # (no such block: the next size class the form admits)
            j += 1
        cases.append((S, K, form, _nodes(N_SPECS[j % 5], form, TB), BETAS[(i // 2) % 2], ETS[(i + i // 6) % 2],
                      MODES[(i + i // 4) % 4], AS[(i + i // 5) % 5]))
    cases.append((8, 64, "explicit8", 129, 1.3, 3, "argmax", 16))
    return cases


MATRIX = _matrix()


def test_matrix_covers_what_it_claims():
    for col, values in ((0, SS), (1, KS), (2, FORMS), (5, ETS), (7, AS)):
        assert set(c[col] for c in MATRIX) == set(values), col
    sizes = set()
    for S, K, form, n, *_ in MATRIX:
        TB = _tile_threads(K)
        sizes |= {spec for spec in N_SPECS if _nodes(spec, form, TB) == n}
    assert sizes == set(N_SPECS)
    assert (8, 64, "explicit8", 129, 1.3, 3, "argmax", 16) in MATRIX


@pytest.mark.parametrize("S,K,form,n,beta,et,mode,A", MATRIX)
def test_form_matrix_against_reference(S, K, form, n, beta, et, mode, A):
    _check_case(_case(S, K, form, n, beta, et, mode), A, 100 * K + 10 * S + A)


# ---- (b) the same posterior as posterior_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("S,K,form,n,et", [(4, 7, "grid_diag", 276, 3), (3, 16, "ragged4", 257, 0)])
def test_identity_tables_give_posterior_kernel_s_posteriors_bit_for_bit(S, K, form, n, et):
    """G = 0, c[k, a] = [k == a]: mean[a] = fmaf(p_a, 1, 0) = p_a, the float32 posterior that posterior_kernel writes"""
    c = _case(S, K, form, n, 1.3, et, "argmax")
    affine = np.zeros((K, K, S + 1))
    affine[np.arange(K), np.arange(K), 0] = 1.0
    b = c.block()
    _, _, post = b.posterior_stats(c.beta, c.et, want_posteriors=True)
    mean, sd = b.ancestral(c.beta, c.et, affine, np.zeros((K, K)))
    b.close()
    assert np.array_equal(mean.astype(np.float64), post.T)
    _compare("identity tables", mean, sd, c.post, c.labels, c.X, affine, np.zeros((K, K)), "posterior")     # sd^2 = p (1 - p)


# ---- (c) the second trip of the grid-stride loop ---------------------------------------------------------------------
def test_second_trip_of_the_grid_stride_loop():
    """more owned nodes than 2048 workgroups of 256 rows: workgroups 0 and 1 take a second tile (the last one partial)"""
    n = ANC_GRID_CAP * 256 + 300
    c = _case(2, 2, "grid_rect", n, 1.3, 3, "argmax")
    assert c.n == n and c.geom[0] * c.geom[1] == n
    affine, cv = _tables(np.random.default_rng(9), 2, 2, 2)
    b = c.block()
    for weighting in WEIGHTINGS:
        mean, sd = b.ancestral(c.beta, c.et, affine, cv, weighting)
        _compare("second trip", mean, sd, c.post, c.labels, c.X, affine, cv, weighting)
        ref_m, _ = AR.reconstruct(c.post, c.labels, c.X, affine, cv, weighting)
        bm, _ = AR.bounds(c.post, c.labels, c.X, affine, cv, weighting)
        for tile in (slice(0, 256), slice(ANC_GRID_CAP * 256, n)):           # the first tile and the second trip's nodes
            assert np.all(np.abs(mean[:, tile] - ref_m[:, tile]) <= bm[:, tile])
            assert np.any(mean[:, tile] != 0)
    b.close()


# ---- (d) row tiles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diagonal", [True, False])
def test_row_tiles_planes_equal_unsplit(diagonal):
    """a block split into two row tiles with halos: the tiles' owned planes, concatenated, are the unsplit block's, bit for bit"""
    from phylo_hmrf_amd import Block, tiles
    N, K, S, A = 90, 12, 4, 5
    blk = synth.make_block(seed=21, H=N, W=N, S=S, K=K, diagonal=diagonal)
    X, e = blk["X"], blk["edges"]
    n = X.shape[0]
    rng = np.random.default_rng(5)
    lp = rng.normal(0.0, 3.0, (n, K))
    labels = blk["labels_true"].astype(np.int64)
    affine, cv = _tables(rng, K, A, S)
    w, eid = R.edge_weights_from_distance(e, 0.5)
    b = Block(n, S, K)
    b.set_observations(X)
    b.set_graph(eid, w)
    b.set_grid(N, N, diagonal, 8)
    b.set_logprob(lp)
    b.set_labels(labels)
    ref = {wt: b.ancestral(1.0, 3, affine, cv, wt) for wt in WEIGHTINGS}
    b.close()
    rows = tiles.split_rows(N, N, diagonal, 2)

    def load(tl):
        tl.b.set_observations(X[tl.global_slice()])

    grp = tiles.make_group(0, (N, N, diagonal), rows, [0, 0], 0, S, K, Block, load, None, 8, 0.5, edges=e)
    got = {wt: ([], []) for wt in WEIGHTINGS}
    for t in sorted(grp.local):
        tl = grp.local[t]
        tl.b.set_logprob(lp[tl.global_slice()])
        tl.b.set_labels(labels[tl.global_slice()])
        g = tl.owned_global_slice()
        for wt in WEIGHTINGS:
            mean, sd = tl.b.ancestral(1.0, 3, affine, cv, wt)
            assert mean.shape == sd.shape == (A, g.stop - g.start)
            got[wt][0].append(mean)
            got[wt][1].append(sd)
        tl.b.close()
    for wt in WEIGHTINGS:
        assert np.array_equal(np.concatenate(got[wt][0], axis=1), ref[wt][0]), wt
        assert np.array_equal(np.concatenate(got[wt][1], axis=1), ref[wt][1]), wt


# ---- (e) determinism ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,K,form,n,A", [(4, 20, "grid_diag", 528, 4), (3, 33, "isolated", 513, 7)])
def test_two_calls_are_bit_identical_and_sd_is_optional(S, K, form, n, A):
    c = _case(S, K, form, n, 1.3, 3, "argmax")
    affine, cv = _tables(np.random.default_rng(3), K, A, S)
    b = c.block()
    for weighting in WEIGHTINGS:
        m1, s1 = b.ancestral(c.beta, c.et, affine, cv, weighting)
        m2, s2 = b.ancestral(c.beta, c.et, affine, cv, weighting)
        m3, s3 = b.ancestral(c.beta, c.et, affine, cv, weighting, want_sd=False)
        assert np.array_equal(m1, m2) and np.array_equal(s1, s2)
        assert s3 is None and np.array_equal(m3, m1)
    b.close()


# ---- (f) the status codes -------------------------------------------------------------------------------------------------
def _raw(b, weighting, A, affine, cv, mean, sd=None):
    import ctypes
    from phylo_hmrf_amd._lib import ptr_d
    fp = ctypes.POINTER(ctypes.c_float)
    return b._L.phmrf_ancestral(b._h, 1.0, 0, int(weighting), int(A), None if affine is None else ptr_d(affine),
                                None if cv is None else ptr_d(cv), None if mean is None else mean.ctypes.data_as(fp),
                                None if sd is None else sd.ctypes.data_as(fp))


def test_status_codes():
    from phylo_hmrf_amd import Block
    c = _case(3, 7, "ragged4", 65, 1.3, 0, "random")
    K, S, A, n = 7, 3, 2, 65
    affine, cv = np.ones((K, A, S + 1)), np.ones((K, A))
    mean = np.zeros((A, n), dtype=np.float32)
    b = c.block()
    assert _raw(b, 0, A, affine, cv, mean) == OK and _raw(b, 1, A, affine, cv, mean) == OK
    # PHMRF_ERR_INVALID: a NULL argument, non-finite tables, a negative cond_var, a weighting other than 0 or 1
    assert b._L.phmrf_ancestral(None, 1.0, 0, 0, A, affine.ctypes.data_as(b._L.phmrf_ancestral.argtypes[5]),
                                cv.ctypes.data_as(b._L.phmrf_ancestral.argtypes[6]),
                                mean.ctypes.data_as(b._L.phmrf_ancestral.argtypes[7]), None) == ERR_INVALID
    assert _raw(b, 0, A, None, cv, mean) == ERR_INVALID
    assert _raw(b, 0, A, affine, None, mean) == ERR_INVALID
    assert _raw(b, 0, A, affine, cv, None) == ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf, 1e39):                  # (1e39 is finite in float64 and not in float32)
        t = affine.copy()
        t[K - 1, A - 1, S] = bad
        assert _raw(b, 0, A, t, cv, mean) == ERR_INVALID, bad
    for bad in (-1e-9, np.nan, np.inf):
        t = cv.copy()
        t[K - 1, A - 1] = bad
        assert _raw(b, 1, A, affine, t, mean) == ERR_INVALID, bad
    for bad in (-1, 2):
        assert _raw(b, bad, A, affine, cv, mean) == ERR_INVALID, bad
    # PHMRF_ERR_UNSUPPORTED: A outside [1, 16], S > 8
    big_a, big_cv = np.ones((K, 17, S + 1)), np.ones((K, 17))
    assert _raw(b, 0, 0, affine, cv, mean) == ERR_UNSUPPORTED
    assert _raw(b, 0, 17, big_a, big_cv, np.zeros((17, n), dtype=np.float32)) == ERR_UNSUPPORTED
    assert _raw(b, 0, 16, big_a, big_cv, np.zeros((16, n), dtype=np.float32)) == OK
    with pytest.raises(ValueError):
        b.ancestral(1.0, 0, affine, cv, weighting="both")
    with pytest.raises(ValueError):
        b.ancestral(1.0, 0, affine[:, :, :S], cv)
    b.close()
    b9 = Block(50, 9, 2)
    b9.set_observations(np.ones((50, 9)))
    b9.set_labels(np.zeros(50, dtype=np.int64))
    assert _raw(b9, 1, 1, np.ones((2, 1, 10)), np.ones((2, 1)), np.zeros((1, 50), dtype=np.float32)) == ERR_UNSUPPORTED
    b9.close()
    # PHMRF_ERR_STATE: no observations, no labels, (posterior only) no log-likelihoods
    b = Block(n, S, K)
    assert _raw(b, 1, A, affine, cv, mean) == ERR_STATE
    b.set_observations(c.X)
    assert _raw(b, 1, A, affine, cv, mean) == ERR_STATE
    b.set_labels(c.labels)
    assert _raw(b, 1, A, affine, cv, mean) == OK                 # (the called state's map needs neither logprob nor a graph)
    assert _raw(b, 0, A, affine, cv, mean) == ERR_STATE
    b.set_graph(c.eid, c.w)
    assert _raw(b, 0, A, affine, cv, mean) == ERR_STATE
    b.set_logprob(c.lp)
    assert _raw(b, 0, A, affine, cv, mean) == OK
    b.close()


# ---- (g) end to end on simulated ancestors ---------------------------------------------------------------------------
def _len_row(n, start, H, W, diag):
    return [n, start, start + n, H, W, 0, 0, 0, 1 if diag else 0, 1]


def _simulated(seed=12, side=48, K=3):
    """a label image, all tree nodes simulated by the recursion per node under its state's parameters, the leaves plus
    min_covar noise (rounded to float32, as the device holds them) as X"""
    from phylo_hmrf_amd import synthetic
    from phylo_hmrf_amd.tree import PhyloTree
    from tests.test_gpu_segment import MIN_COVAR
    rng = np.random.default_rng(seed)
    tree = PhyloTree(synthetic.tree_for(4))
    params = synthetic.sample_ou_params(rng, tree, K)
    lab = synthetic.label_image(rng, side, side, K).reshape(-1)
    n = len(lab)
    Z = np.zeros((n, tree.node_num))
    for k in range(K):
        at = np.flatnonzero(lab == k)
        Z[at] = AR.simulate(tree, params[k], len(at), rng)
    X = _f32(Z[:, tree.leaf_vec] + np.sqrt(MIN_COVAR) * rng.standard_normal((n, 4)))
    return tree, params, lab, Z, X, R.grid_edges(X, side, side, False, 8)


def test_end_to_end_reconstructs_simulated_ancestors():
    from phylo_hmrf_amd import ancestral
    from phylo_hmrf_amd.hmrf import phyloHMRF
    from tests.test_gpu_segment import MIN_COVAR, _model
    tree, params, lab_true, Z, X, edges = _simulated()
    n, K = len(lab_true), len(params)
    model = _model(K, params)
    A_nodes = tree.internal_nodes
    affine, cv = (_f32(t) for t in tree.ancestral_tables(params, MIN_COVAR))
    prior = tree.node_moments(params)[0][:, A_nodes]                        # m_A per state
    w, eid = R.edge_weights_from_distance(edges, 0.5)
    truth = Z[:, A_nodes].T

    def mse(planes):
        return float(np.mean((planes - truth) ** 2))

    # the condition on these inputs, in float64 on the true labels: conditioning on the leaves beats the state's prior mean
    lp64 = R.log_multivariate_normal_density_full(X, model.means_, model._covars_)
    post64 = P.posteriors_costs_stats(lab_true, lp64, X, eid, w, model.beta, model.estimate_type)[0]
    for weighting in WEIGHTINGS:
        ref_m, _ = AR.reconstruct(post64, lab_true, X, affine, cv, weighting)
        print("float64, true labels, %s: mse %.4f, prior mean %.4f" % (weighting, mse(ref_m), mse(prior[lab_true].T)))
        assert mse(ref_m) < mse(prior[lab_true].T)

    m = phyloHMRF.from_model(model, X, [_len_row(n, 0, 48, 48, False)], [edges], quiet=True)
    try:
        with pytest.raises(RuntimeError):
            m.ancestral()                                                    # no labels on the device yet
        seg = m.segment()
        res = {wt: m.ancestral(weighting=wt) for wt in WEIGHTINGS}
        lp_dev = m.blocks[0].get_logprob()                                   # what the kernel read: the bounds take the posteriors from it
    finally:
        m.close()
    lab = seg["state_vec"].astype(np.int64)
    post = P.posteriors_costs_stats(lab, lp_dev, X, eid, w, model.beta, model.estimate_type)[0]
    at, cv_model = ancestral.model_tables(model)
    assert np.array_equal(_f32(at), affine) and np.array_equal(_f32(cv_model), cv)
    for wt in WEIGHTINGS:
        r = res[wt]
        assert r["nodes"].tolist() == A_nodes.tolist() and r["parent"].tolist() == tree.parent.tolist()
        assert r["mean"].shape == r["sd"].shape == (len(A_nodes), n)
        _compare("end to end", r["mean"], r["sd"], post, lab, X, affine, cv, wt)
        print("device, %s: mse %.4f, prior mean of the called state %.4f" % (wt, mse(r["mean"]), mse(prior[lab].T)))
        assert mse(r["mean"].astype(np.float64)) < mse(prior[lab].T)
        assert set(r["timing"]) == {"emission", "ancestral"}
    no_sd = None
    m = phyloHMRF.from_model(model, X, [_len_row(n, 0, 48, 48, False)], [edges], quiet=True)
    try:
        m.segment()
        no_sd = m.ancestral(want_sd=False)
    finally:
        m.close()
    assert no_sd["sd"] is None and np.array_equal(no_sd["mean"], res["posterior"]["mean"])


# ---- (h) the command line ----------------------------------------------------------------------------------------------------
def _cli(out, seed, extra):
    import phylo_hmrf as cli
    return cli.run("4", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", out, synthetic="48",
                   seed=str(seed), quiet="1", **extra)


def test_cli_segment_then_ancestral(tmp_path):
    import scipy.io
    from phylo_hmrf_amd import ancestral, model_io
    fit_dir, seg_dir = str(tmp_path / "fit"), str(tmp_path / "seg")
    mpath = str(tmp_path / "m.npz")
    _cli(fit_dir, 7, dict(save_model=mpath))
    f = _cli(seg_dir, 8, dict(segment=mpath, ancestral="posterior"))
    assert os.path.basename(f) == "segment_0_4.mat"
    seg = scipy.io.loadmat(f)
    assert sorted(k for k in seg if not k.startswith("__")) == ["conf", "energy", "len_vec", "state_vec", "top"]
    path = os.path.join(seg_dir, "ancestral_0_4.npz")
    assert os.path.exists(path)
    d = ancestral.load_npz(path)
    tree = model_io.load_model(mpath).tree
    n = seg["state_vec"].size
    assert d["nodes"].tolist() == tree.internal_nodes.tolist() and d["parent"].tolist() == tree.parent.tolist()
    assert d["mean"].shape == (len(tree.internal_nodes), n) and d["mean"].dtype == np.float32
    assert d["sd"].shape == d["mean"].shape and np.all(np.isfinite(d["sd"])) and np.all(d["sd"] >= 0)
    assert np.all(np.isfinite(d["mean"])) and d["weighting"] == "posterior"
    assert np.array_equal(d["len_vec"], seg["len_vec"])


# ---- (i) two ranks on one GPU ------------------------------------------------------------------------------------------------
ANC_WORKER = r'''
import os, sys, json
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
world = int(os.environ.get("WORLD_SIZE", "1"))
if world > 1:
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=world)
from oracle import synth
from phylo_hmrf_amd.hmrf import phyloHMRF
from test_gpu_segment import _model
blk_a = synth.make_block(41, 120, 120, 4, 8, True)
blk_b = synth.make_block(42, 40, 40, 4, 8, True)
X = np.concatenate([blk_a["X"], blk_b["X"]])
na, nb = blk_a["X"].shape[0], blk_b["X"].shape[0]
lv = [[na, 0, na, 120, 120, 0, 0, 0, 1, 1], [nb, na, na + nb, 40, 40, 0, 0, 1, 1, 1]]
m = phyloHMRF.from_model(_model(8, blk_a["params"], energy_tol_ppb=0), X, lv, [blk_a["edges"], blk_b["edges"]], quiet=True, split_above=0.6)
seg = m.segment()
out = dict(split=[int(r) for r in m.split_regions], state_vec=seg["state_vec"].astype(int).tolist())
for wt in ("posterior", "called"):
    res = m.ancestral(weighting=wt)
    out[wt] = dict(mean=res["mean"].view(np.int32).tolist(), sd=res["sd"].view(np.int32).tolist())
m.close()
if int(os.environ.get("RANK", "0")) == 0:
    json.dump(out, open(%(out)r, "w"))
if world > 1:
    dist.barrier()
    dist.destroy_process_group()
'''


def _run_ranks(tmp_path, world, port):
    out = str(tmp_path / ("anc_w%d.json" % world))
    script = tmp_path / ("anc_worker_w%d.py" % world)
    script.write_text(ANC_WORKER % {"root": ROOT, "out": out})
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      cwd=ROOT))
    for p in procs:
        o, _ = p.communicate(timeout=900)
        assert p.returncode == 0, o.decode()[-3000:]
    return json.load(open(out))


def test_two_ranks_planes_like_one(tmp_path):
    """the large block is cut into row tiles on two ranks, which settle in a labelling of their own
    (test_two_ranks_segment_like_one): the planes the two ranks gather are, bit for bit, the planes one rank computes on
    that gathered labelling with whole blocks"""
    from phylo_hmrf_amd import Block, ancestral
    from tests.test_gpu_segment import _model
    two = _run_ranks(tmp_path, 2, 29653)
    assert two["split"] == [0]
    blocks = [synth.make_block(41, 120, 120, 4, 8, True), synth.make_block(42, 40, 40, 4, 8, True)]
    m = _model(8, blocks[0]["params"])
    affine, cv = ancestral.model_tables(m)
    lab = np.asarray(two["state_vec"], dtype=np.int64)
    start = 0
    for blk, N in zip(blocks, (120, 40)):
        n = blk["X"].shape[0]
        b = Block(n, 4, 8)
        ew, weid = R.edge_weights_from_distance(blk["edges"], 0.5)
        b.set_graph(weid, ew)
        b.set_grid(N, N, True, 8)
        b.set_observations(blk["X"])
        b.emission(m.means_, m._covars_)
        b.set_labels(lab[start:start + n])
        for wt in WEIGHTINGS:
            mean, sd = b.ancestral(m.beta, m.estimate_type, affine, cv, wt)
            got_m = np.asarray(two[wt]["mean"], dtype=np.int32).view(np.float32)[:, start:start + n]
            got_s = np.asarray(two[wt]["sd"], dtype=np.int32).view(np.float32)[:, start:start + n]
            assert np.array_equal(got_m, mean) and np.array_equal(got_s, sd), (N, wt)
        b.close()
        start += n
