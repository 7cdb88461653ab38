"""GPU: segmenting new data with a saved model -- the posterior summary kernel (phmrf_posterior_summary) against the f64
oracle, on row tiles, the segmentation's energy against gco's swap from the same argmax start, the command line end to
end, and two ranks on one GPU over gloo."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref_numpy as R
from oracle import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
MIN_COVAR = 2e-3


def _block(n, S, K):
    from phylo_hmrf_amd import Block
    return Block(n, S, K)


def _oracle_summary(labels, lp, eid, w, beta, estimate_type):
    post = R.compute_posteriors_graph(labels, lp, eid, w, R.potts_matrix(lp.shape[1], beta), estimate_type)[0]
    idx = np.arange(lp.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.sum(np.where(post > 0, post * np.log(post), 0.0), axis=1)
    return post, post[idx, labels], ent


def _ragged_graph(rng, n, max_deg=4):
    """a random simple graph of degree <= max_deg (D = 4 adjacency rows, many of them ragged) with node 0 isolated"""
    deg = np.zeros(n, dtype=np.int64)
    seen, out = set(), []
    for _ in range(3 * n):
        a, b = (int(v) for v in rng.integers(1, n, 2))
        if a == b or deg[a] >= max_deg or deg[b] >= max_deg or (min(a, b), max(a, b)) in seen:
            continue
        seen.add((min(a, b), max(a, b)))
        deg[a] += 1
        deg[b] += 1
        out.append((min(a, b), max(a, b)))
    return np.asarray(out, dtype=np.int64), rng.uniform(0.2, 1.0, len(out))


def _check_against_oracle(b, labels, lp, eid, w, beta, et):
    conf, top, ent = b.posterior_summary(beta, et, want_entropy=True)
    post, conf_ref, ent_ref = _oracle_summary(labels, lp, eid, w, beta, et)
    assert conf.dtype == np.float32 and top.dtype == np.uint8 and ent.dtype == np.float32
    assert np.max(np.abs(conf - conf_ref)) < 2e-5
    assert np.max(np.abs(ent - ent_ref)) < 1e-4
    srt = np.sort(post, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 1e-5 if post.shape[1] > 1 else np.ones(post.shape[0], dtype=bool)
    assert np.array_equal(top[clear], np.argmax(post, axis=1)[clear])
    # the same posteriors as the statistics kernel's, for the called state
    _, _, post_dev = b.posterior_stats(beta, et, want_posteriors=True)
    assert np.max(np.abs(conf.astype(np.float64) - post_dev[np.arange(len(labels)), labels])) <= 1e-7
    c2, t2, e2 = b.posterior_summary(beta, et)           # (no entropy: the other outputs do not change)
    assert e2 is None and np.array_equal(c2, conf) and np.array_equal(t2, top)


@pytest.mark.parametrize("K", [1, 2, 5, 20, 64])
@pytest.mark.parametrize("et", [0, 3])
@pytest.mark.parametrize("form", ["grid", "explicit8", "ragged4"])
def test_summary_matches_oracle(K, et, form):
    rng = np.random.default_rng(100 * K + 10 * et + len(form))
    beta = 1.3
    if form == "ragged4":
        n = 1237
        eid, w = _ragged_graph(rng, n)
    else:
        N = 61 if K != 64 else 47                       # n = 1891 / 1128: not a multiple of the 256 / 128-row tile
        blk = synth.make_block(seed=K + et, H=N, W=N, S=4, K=max(K, 2), diagonal=True)
        w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
        n = blk["X"].shape[0]
    lp = rng.normal(0.0, 3.0, (n, K)) - 5.0
    labels = rng.integers(0, K, n)
    b = _block(n, 4, K)
    b.set_observations(rng.random((n, 4)))
    b.set_graph(eid, w)
    if form == "grid":
        b.set_grid(N, N, True, 8)
    b.set_logprob(lp)
    b.set_labels(labels)
    _check_against_oracle(b, labels, lp.astype(np.float32).astype(np.float64), eid, w, beta, et)
    b.close()


def test_summary_needs_labels_and_logprob():
    from phylo_hmrf_amd._lib import PhmrfError
    blk = synth.make_block(seed=2, H=20, W=20, S=4, K=3, diagonal=True)
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    n = blk["X"].shape[0]
    b = _block(n, 4, 3)
    b.set_graph(eid, w)
    with pytest.raises(PhmrfError) as e:
        b.posterior_summary(1.0, 0)
    assert e.value.status == 5
    b.set_logprob(np.zeros((n, 3)))
    with pytest.raises(PhmrfError) as e:
        b.posterior_summary(1.0, 0)
    assert e.value.status == 5
    b.close()


@pytest.mark.parametrize("diagonal", [True, False])
def test_row_tiles_summary_equals_unsplit(diagonal):
    """a block split into two row tiles with halos: each tile's owned-row summary is the unsplit block's"""
    from phylo_hmrf_amd import Block, tiles
    N, K = 90, 12
    blk = synth.make_block(seed=21, H=N, W=N, S=4, K=K, diagonal=diagonal)
    X, e = blk["X"], blk["edges"]
    n = X.shape[0]
    rng = np.random.default_rng(5)
    lp = rng.normal(0.0, 3.0, (n, K))
    labels = blk["labels_true"].astype(np.int64)
    w, eid = R.edge_weights_from_distance(e, 0.5)
    b = _block(n, 4, K)
    b.set_graph(eid, w)
    b.set_grid(N, N, diagonal, 8)
    b.set_logprob(lp)
    b.set_labels(labels)
    ref = b.posterior_summary(1.0, 3, want_entropy=True)
    b.close()
    rows = tiles.split_rows(N, N, diagonal, 2)

    def load(tl):
        tl.b.set_observations(X[tl.global_slice()])

    grp = tiles.make_group(0, (N, N, diagonal), rows, [0, 0], 0, 4, K, Block, load, None, 8, 0.5, edges=e)
    covered = 0
    for t in sorted(grp.local):
        tl = grp.local[t]
        tl.b.set_logprob(lp[tl.global_slice()])
        tl.b.set_labels(labels[tl.global_slice()])
        conf, top, ent = tl.b.posterior_summary(1.0, 3, want_entropy=True)
        g = tl.owned_global_slice()
        assert conf.shape == (g.stop - g.start,)
        assert np.array_equal(top, ref[1][g])
        assert np.max(np.abs(conf - ref[0][g])) <= 1e-7
        assert np.max(np.abs(ent - ref[2][g])) <= 1e-7
        covered += conf.size
        tl.b.close()
    assert covered == n


# ---- the segmentation's energy against gco's swap from the same argmax start ----------------------------------------------
def _model(K, params, beta=1.0, estimate_type=0, energy_tol_ppb=10000):
    from phylo_hmrf_amd import model_io, synthetic
    from phylo_hmrf_amd.tree import PhyloTree
    tree = PhyloTree(synthetic.tree_for(4))
    means, covars = tree.mean_cov(params, MIN_COVAR)
    return model_io.Model(K=K, S=4, edge_list=np.asarray(synthetic.tree_for(4), dtype=np.int64), branch_list=None, species=None,
                          means_=means, _covars_=covars, params_vec=np.asarray(params), params_vec1=np.asarray(params),
                          min_covar=MIN_COVAR, beta=beta, beta1=0.5, estimate_type=estimate_type, num_neighbor=8,
                          energy_tol_ppb=energy_tol_ppb, x_max=float("nan"), resolution=-1, filter_mode=-1,
                          filter_sigma=float("nan"), diagonal_type=-1, tree=tree)


def _len_row(n, start, N, diag):
    return [n, start, start + n, N, N, 0, 0, 0, 1 if diag else 0, 1]


SEGMENT_GCO_CASES = [(0, 150, 10, False), (1, 160, 20, True), (5, 220, 20, True), (11, 652, 20, True)]


@pytest.mark.parametrize("seed,N,K,diagonal", SEGMENT_GCO_CASES)
def test_segment_energy_at_or_below_gco_swap_from_argmax(seed, N, K, diagonal):
    from oracle import gco_ref
    from phylo_hmrf_amd.hmrf import phyloHMRF
    sys.path.insert(0, G)
    import make_golden_segment_gco as mk
    blk, means, covars, eid, w, lp, init = mk.case_inputs(seed, N, K, diagonal)
    n = lp.shape[0]
    rec = [c for c in json.load(open(os.path.join(G, "segment_gco_energies.json")))["cases"]
           if (c["seed"], c["N"], c["K"], c["diagonal"]) == (seed, N, K, bool(diagonal))]
    assert len(rec) == 1, "no recorded gco energies for this case: run tests/golden/make_golden_segment_gco.py"
    np.testing.assert_allclose(R.mrf_energy(init, lp, eid, w, 1.0)[0], rec[0]["e_init"], rtol=1e-12)
    e_ref = {"pygco": rec[0]["e_pygco"], "fine": rec[0]["e_fine"]}
    if gco_ref.available():
        V = R.potts_matrix(K, 1.0)
        for q in ("pygco", "fine"):
            lab = gco_ref.cut_general_graph(eid, w, -lp, V, n_iter=5000, algorithm="swap", init_labels=init, quant=q)
            np.testing.assert_allclose(R.mrf_energy(lab, lp, eid, w, 1.0)[0], e_ref[q], rtol=1e-12)
    m = phyloHMRF.from_model(_model(K, blk["params"]), blk["X"], [_len_row(n, 0, N, diagonal)], [blk["edges"]], quiet=True)
    try:
        res = m.segment(want_entropy=True)
    finally:
        m.close()
    lab = res["state_vec"].astype(np.int64)
    assert res["state_vec"].dtype == np.float64 and lab.shape == (n,)
    e_mine = R.mrf_energy(lab, lp, eid, w, 1.0)[0]
    print("n %d K %d: segmentation %.3f  gco swap pygco %.3f  fine %.3f" % (n, K, e_mine, e_ref["pygco"], e_ref["fine"]))
    np.testing.assert_allclose(res["energy"][0], e_mine, rtol=1e-5)
    assert e_mine < e_ref["pygco"]
    assert e_mine <= e_ref["fine"] + 1e-5 * abs(e_ref["fine"])
    assert np.all(res["conf"] > 0) and np.all(res["conf"] <= 1)
    assert np.all(res["entropy"] >= 0) and np.all(res["entropy"] <= np.log(K) + 1e-4)


# ---- end to end ------------------------------------------------------------------------------------------------------
def _cli(out, seed, extra):
    import phylo_hmrf as cli
    return cli.run("4", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", out, synthetic="64",
                   seed=str(seed), quiet="1", **extra)


def test_cli_save_model_then_segment_other_data(tmp_path, monkeypatch):
    import scipy.io
    from phylo_hmrf_amd import kmeans, model_io, mstep
    fit_dir, seg_dir = str(tmp_path / "fit"), str(tmp_path / "seg")
    mpath = str(tmp_path / "m.npz")
    _cli(fit_dir, 7, dict(save_model=mpath))
    z = model_io.load_model(mpath)
    assert (z.K, z.S) == (4, 4) and np.isnan(z.x_max)

    def boom(*a, **k):
        raise AssertionError("fit work in a segment run")

    for mod, name in ((kmeans, "minibatch_centers"), (kmeans, "device_kmeans"), (kmeans, "device_moments"),
                      (mstep, "do_mstep"), (mstep, "init_ou_params"), (mstep, "init_ou_params_moments")):
        monkeypatch.setattr(mod, name, boom)
    f = _cli(seg_dir, 8, dict(segment=mpath))
    assert mstep._POOL is None                                  # (no M-step worker pool either)
    assert os.path.basename(f) == "segment_0_4.mat" and os.path.exists(f)
    assert not [p for p in os.listdir(seg_dir) if p.startswith("estimate_ou_")]
    d = scipy.io.loadmat(f)
    for k in ("state_vec", "len_vec", "conf", "top", "energy"):
        assert k in d, k
    n = 64 * 65 // 2
    assert d["state_vec"].size == n and d["conf"].size == n and d["top"].size == n
    assert np.all(d["conf"] > 0) and np.all(d["conf"] <= 1)
    assert np.all(np.isfinite(d["energy"]))
    assert set(np.unique(d["state_vec"]).astype(int)) <= set(range(4))


def test_two_regions_equal_each_alone(monkeypatch):
    monkeypatch.setenv("PHMRF_DETERMINISTIC", "1")
    from phylo_hmrf_amd.hmrf import phyloHMRF
    blocks = [synth.make_block(31, 70, 70, 4, 6, True), synth.make_block(32, 50, 60, 4, 6, False)]
    model = _model(6, blocks[0]["params"])
    geo = [(70, 70, 1), (50, 60, 0)]
    alone = []
    for blk, (H, W, diag) in zip(blocks, geo):
        n = blk["X"].shape[0]
        m = phyloHMRF.from_model(model, blk["X"], [[n, 0, n, H, W, 0, 0, 0, diag, 1]], [blk["edges"]], quiet=True)
        alone.append(m.segment(want_entropy=True))
        m.close()
    X = np.concatenate([b["X"] for b in blocks])
    n0, n1 = blocks[0]["X"].shape[0], blocks[1]["X"].shape[0]
    lv = [[n0, 0, n0, 70, 70, 0, 0, 0, 1, 1], [n1, n0, n0 + n1, 50, 60, 0, 0, 1, 0, 1]]
    m = phyloHMRF.from_model(model, X, lv, [b["edges"] for b in blocks], quiet=True)
    both = m.segment(want_entropy=True)
    m.close()
    for key in ("state_vec", "conf", "top", "entropy"):
        assert np.array_equal(both[key], np.concatenate([alone[0][key], alone[1][key]])), key
    assert np.array_equal(both["energy"], np.array([alone[0]["energy"][0], alone[1]["energy"][0]]))


# ---- two ranks on one GPU ------------------------------------------------------------------------------------------------
SEG_WORKER = r'''
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
res = m.segment()
out = dict(split=[int(r) for r in m.split_regions], state_vec=res["state_vec"].astype(int).tolist(),
           conf=res["conf"].view(np.int32).tolist(), top=res["top"].astype(int).tolist(), energy=res["energy"].tolist())
m.close()
if int(os.environ.get("RANK", "0")) == 0:
    json.dump(out, open(%(out)r, "w"))
if world > 1:
    dist.barrier()
    dist.destroy_process_group()
'''


def _run_seg(tmp_path, world, port):
    out = str(tmp_path / ("seg_w%d.json" % world))
    script = tmp_path / ("seg_worker_w%d.py" % world)
    script.write_text(SEG_WORKER % {"root": ROOT, "out": out})
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


def test_two_ranks_segment_like_one(tmp_path):
    one = _run_seg(tmp_path, 1, 29641)
    two = _run_seg(tmp_path, 2, 29643)
    assert one["split"] == [] and two["split"] == [0]          # the large block is cut into row tiles on two ranks
    blk_a = synth.make_block(41, 120, 120, 4, 8, True)
    blk_b = synth.make_block(42, 40, 40, 4, 8, True)
    m = _model(8, blk_a["params"])
    X = np.concatenate([blk_a["X"], blk_b["X"]])
    lp = R.log_multivariate_normal_density_full(X, m.means_, m._covars_)
    na = blk_a["X"].shape[0]
    e_b = blk_b["edges"].copy()
    e_b[:, :2] += na
    w, eid = R.edge_weights_from_distance(np.concatenate([blk_a["edges"], e_b]), 0.5)
    e1 = R.mrf_energy(np.asarray(one["state_vec"]), lp, eid, w, 1.0)[0]
    e2 = R.mrf_energy(np.asarray(two["state_vec"]), lp, eid, w, 1.0)[0]
    # (row tiles pin the rows at their cuts in turn and settle in another local optimum than the unsplit block: measured
    #  3.6e-5 of |E| apart at the default 1e-5 stopping tolerance on this 7,260-node block cut in three; both solved to the
    #  exact fixed point here)
    assert abs(e2 - e1) <= 1e-4 * abs(e1), (e1, e2)
    np.testing.assert_allclose(sum(two["energy"]), e2, rtol=1e-5)
    # the gathered conf / top are the summary of the gathered labelling, recomputed on one rank
    lab = np.asarray(two["state_vec"], dtype=np.int64)
    conf2 = np.asarray(two["conf"], dtype=np.int32).view(np.float32)
    from phylo_hmrf_amd import Block
    b = Block(na, 4, 8)
    ew, weid = R.edge_weights_from_distance(blk_a["edges"], 0.5)
    b.set_graph(weid, ew)
    b.set_grid(120, 120, True, 8)
    b.set_observations(blk_a["X"])
    b.emission(m.means_, m._covars_)
    b.set_labels(lab[:na])
    conf, top, _ = b.posterior_summary(1.0, 0)
    b.close()
    assert np.array_equal(top, np.asarray(two["top"][:na], dtype=np.uint8))
    assert np.array_equal(conf, conf2[:na])
