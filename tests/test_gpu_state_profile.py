"""GPU: the state profile's two entry points (phmrf_state_hist, phmrf_state_moments) against their NumPy restatement in
every form the kernels take -- sizes around a wave and a workgroup and past the grid cap, every K / S / J axis value, labels
in long runs and drawn per node, concentrated and scattered data --, on row tiles, from run to run, their error statuses,
and model.state_profile() end to end after a segmentation."""
import numpy as np
import pytest

from oracle import synth
from phylo_hmrf_amd import profile as P
from tests import state_profile_reference as SR

pytestmark = pytest.mark.gpu
SHIFTS = (24, 16, 8, 0)
# every workgroup of the histogram kernel (P.HIST_GRID_CAP of them along x, 256 nodes a trip) makes a second strided trip
N_CAP = 2 * P.HIST_GRID_CAP * 256 - 100


def _block(x, labels, K):
    from phylo_hmrf_amd import Block
    b = Block(x.shape[0], x.shape[1], K)
    b.set_observations(x)
    b.set_labels(labels)
    return b


def _prefixes(rng, x32, labels, K, J, shift):
    """prefix table [K, S, J] for the pass at `shift`: prefixes that occur in the state's own values (so the slots count
    something), among them repeats, and slots holding the sentinel"""
    keys = SR.order_key(x32).astype(np.int64) >> (shift + 8)
    S = x32.shape[1]
    pre = np.full((K, S, J), P.SENTINEL, dtype=np.uint32)
    for k in range(K):
        rows = np.nonzero(labels == k)[0]
        if rows.size == 0:
            pre[k] = rng.integers(0, 1 << 8, (S, J))            # nothing to match: any prefix counts nothing
            continue
        for s in range(S):
            pre[k, s] = keys[rows[rng.integers(0, rows.size, J)], s]
    pre[rng.random((K, S, J)) < 0.2] = P.SENTINEL
    return pre


# (n, K, S, J, labels, data): every value of every axis at least once
HIST_CASES = [
    (1, 1, 1, 1, "runs", "normal"), (1, 3, 4, 3, "nodes", "signs"), (63, 1, 4, 3, "runs", "constant"),
    (63, 3, 5, 16, "nodes", "eighths"), (64, 3, 1, 1, "runs", "topbyte"), (64, 20, 4, 3, "nodes", "normal"),
    (65, 3, 8, 3, "runs", "signs"), (65, 20, 5, 1, "nodes", "constant"), (257, 3, 4, 16, "runs", "eighths"),
    (257, 20, 4, 3, "nodes", "topbyte"), (257, 64, 1, 3, "runs", "normal"), (257, 1, 16, 1, "nodes", "eighths"),
    (1000, 1, 4, 3, "runs", "topbyte"), (1000, 3, 4, 3, "runs", "constant"), (1000, 3, 4, 3, "nodes", "constant"),
    (1000, 20, 4, 3, "runs", "normal"), (1000, 20, 4, 16, "nodes", "signs"), (1000, 20, 5, 3, "runs", "eighths"),
    (1000, 20, 8, 1, "nodes", "topbyte"), (1000, 20, 16, 3, "runs", "normal"), (1000, 64, 4, 3, "runs", "topbyte"),
    (1000, 64, 4, 1, "nodes", "normal"), (1000, 64, 8, 16, "runs", "signs"), (1000, 64, 16, 16, "nodes", "eighths"),
    (1000, 64, 16, 16, "runs", "constant"), (1000, 3, 1, 16, "nodes", "topbyte"), (1000, 1, 5, 16, "runs", "signs"),
    (N_CAP, 3, 1, 3, "runs", "topbyte"), (N_CAP, 20, 4, 1, "runs", "normal"), (N_CAP, 3, 4, 3, "nodes", "constant"),
]


def test_hist_cases_cover_every_axis():
    assert set(c[0] for c in HIST_CASES) == {1, 63, 64, 65, 257, 1000, N_CAP}
    assert set(c[1] for c in HIST_CASES) == {1, 3, 20, 64} and set(c[2] for c in HIST_CASES) == {1, 4, 5, 8, 16}
    assert set(c[3] for c in HIST_CASES) == {1, 3, 16} and set(c[4] for c in HIST_CASES) == {"runs", "nodes"}
    assert set(c[5] for c in HIST_CASES) == set(SR.FORMS)


@pytest.mark.parametrize("n,K,S,J,kind,form", HIST_CASES)
def test_state_hist_equals_reference(n, K, S, J, kind, form):
    rng = np.random.default_rng(n + 7 * K + 11 * S + 13 * J)
    x = SR.make_values(form, rng, n, S)
    labels = SR.make_labels(kind, rng, n, K)
    x32 = x.astype(np.float32)
    b = _block(x, labels, K)
    try:
        for shift in SHIFTS:
            pre = None if shift == 24 else _prefixes(rng, x32, labels, K, J, shift)
            got = b.state_hist(shift, pre)
            want = SR.state_hist(x32, labels, K, shift, pre)
            assert got.dtype == np.uint64 and got.shape == want.shape
            assert np.array_equal(got, want), (shift, np.argwhere(got != want)[:5])
            if shift == 24:
                assert np.array_equal(got.sum(axis=(2, 3)), np.repeat(np.bincount(labels, minlength=K)[:, None], S, axis=1))
            else:
                assert int(want.sum()) > 0 or n < 3
    finally:
        b.close()


# (H, W, diagonal, dist0, K, S, labels, data)
MOMENT_CASES = [
    (50, 50, True, 0, 3, 4, "runs", "normal"), (61, 61, True, 0, 20, 4, "nodes", "eighths"),
    (40, 70, False, 0, 3, 5, "runs", "signs"), (40, 70, False, 37, 20, 4, "runs", "eighths"),
    (33, 90, False, -500, 3, 1, "nodes", "constant"), (70, 40, False, 100000, 64, 4, "runs", "topbyte"),
    (7, 9, False, -3, 1, 16, "nodes", "normal"), (1, 1, True, 0, 1, 1, "runs", "eighths"),
    (64, 64, False, 5, 64, 16, "nodes", "eighths"), (50, 50, True, 0, 64, 8, "runs", "normal"),
]


def _check_moments(got, ref, exact):
    count, total, sq, bands = got
    r_count, r_total, r_sq, a1, a2, r_bands = ref
    assert np.array_equal(count, r_count)
    if r_bands is not None:
        assert np.array_equal(bands, r_bands) and bands.sum() == count.sum()
    if exact:
        assert np.array_equal(total, r_total) and np.array_equal(sq, r_sq)
        return
    # any order of summation of n terms is within (n - 1) 2^-53 sum |term| of the exact sum
    slack = np.maximum(count - 1, 0)[:, None] * 2.0 ** -53
    e1, e2 = np.abs(total - r_total), np.abs(sq - r_sq)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("worst sum error / bound %.3g, sumsq %.3g" % (np.nanmax(np.where(slack * a1 > 0, e1 / (slack * a1), 0.0)),
                                                             np.nanmax(np.where(slack * a2 > 0, e2 / (slack * a2), 0.0))))
    assert np.all(e1 <= slack * a1) and np.all(e2 <= slack * a2)


@pytest.mark.parametrize("H,W,diagonal,dist0,K,S,kind,form", MOMENT_CASES)
def test_state_moments_equal_reference(H, W, diagonal, dist0, K, S, kind, form):
    rng = np.random.default_rng(H + 3 * W + K + S)
    n = H * (H + 1) // 2 if diagonal else H * W
    x = SR.make_values(form, rng, n, S)
    labels = SR.make_labels(kind, rng, n, K)
    b = _block(x, labels, K)
    try:
        ref = SR.state_moments(x.astype(np.float32), labels, K, None, 0)
        got = b.state_moments()                                     # no grid: counts and sums alone
        assert got[3] is None
        _check_moments(got, ref, form == "eighths")
        if n > 1:                                                   # (a single cell: bands on one node say nothing more)
            b.build_grid_graph(H, W, diagonal, 8, 0.5)
            ref = SR.state_moments(x.astype(np.float32), labels, K, (H, W, diagonal), dist0)
            _check_moments(b.state_moments(dist0, want_bands=True), ref, form == "eighths")
    finally:
        b.close()


@pytest.mark.parametrize("diagonal,dist0", [(True, 0), (False, 0), (False, -17)])
def test_row_tiles_add_up_to_the_unsplit_block(diagonal, dist0):
    """a block split into two row tiles with halo rows: histograms, counts and bands of the tiles' owned rows add up"""
    from phylo_hmrf_amd import Block, tiles
    N, K, S = 40, 5, 4
    rng = np.random.default_rng(3 + int(diagonal))
    n = N * (N + 1) // 2 if diagonal else N * N
    x = SR.make_values("eighths", rng, n, S)
    labels = SR.make_labels("runs", rng, n, K)
    x32 = x.astype(np.float32)
    pre = {shift: _prefixes(rng, x32, labels, K, 3, shift) for shift in SHIFTS[1:]}
    rows = tiles.split_rows(N, N, diagonal, 2)

    def load(tl):
        tl.b.set_observations(x[tl.global_slice()])

    grp = tiles.make_group(0, (N, N, diagonal), rows, [0, 0], 0, S, K, Block, load, None, 8, 0.5)
    hist = {shift: 0 for shift in SHIFTS}
    count, total, sq, bands = 0, 0, 0, 0
    try:
        assert len(grp.local) == 2
        for t in sorted(grp.local):
            tl = grp.local[t]
            tl.b.set_labels(labels[tl.global_slice()])
            for shift in SHIFTS:
                hist[shift] = hist[shift] + tl.b.state_hist(shift, pre.get(shift))
            got = tl.b.state_moments(dist0 if diagonal else dist0 - tl.s0, want_bands=True)
            count, total, sq, bands = count + got[0], total + got[1], sq + got[2], bands + got[3]
    finally:
        for tl in grp.local.values():
            tl.b.close()
    for shift in SHIFTS:
        assert np.array_equal(hist[shift], SR.state_hist(x32, labels, K, shift, pre.get(shift))), shift
    ref = SR.state_moments(x32, labels, K, (N, N, diagonal), dist0)
    _check_moments((count, total, sq, bands), ref, True)


def _all_outputs(x, labels, K, H, W):
    b = _block(x, labels, K)
    try:
        b.build_grid_graph(H, W, False, 8, 0.5)
        pre = np.zeros((K, x.shape[1], 2), dtype=np.uint32)
        pre[:, :, 0] = 0xBF                                          # the top byte of the keys of [1, 2)
        pre[:, :, 1] = P.SENTINEL
        return [b.state_hist(24), b.state_hist(16, pre)] + list(b.state_moments(3, want_bands=True))
    finally:
        b.close()


@pytest.mark.parametrize("deterministic", [False, True])
def test_two_calls_return_the_same_bytes(monkeypatch, deterministic):
    """integer outputs always; sum and sumsq under PHMRF_DETERMINISTIC=1 (there is one path: without it too), on data whose
    sums depend on the order of the additions"""
    if deterministic:
        monkeypatch.setenv("PHMRF_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("PHMRF_DETERMINISTIC", raising=False)
    rng = np.random.default_rng(8)
    H, W, K = 90, 110, 7
    x = 1.0 + 0.96 * rng.random((H * W, 4)) * np.exp(rng.normal(0.0, 0.2, (H * W, 4)))
    labels = SR.make_labels("runs", rng, H * W, K)
    labels[::7] = rng.integers(0, K, labels[::7].size)
    one, two = _all_outputs(x, labels, K, H, W), _all_outputs(x, labels, K, H, W)
    for a, c in zip(one, two):
        assert a.tobytes() == c.tobytes()
    assert one[1].sum() > 0


def test_error_statuses():
    from phylo_hmrf_amd import Block
    from phylo_hmrf_amd._lib import PhmrfError
    K, S, n = 3, 2, 30
    b = Block(n, S, K)
    try:
        def status(fn):
            with pytest.raises(PhmrfError) as e:
                fn()
            return e.value.status

        assert status(lambda: b.state_hist(24)) == 5               # no observations
        assert status(lambda: b.state_moments()) == 5
        b.set_observations(np.zeros((n, S)))
        assert status(lambda: b.state_hist(24)) == 5               # no labels
        assert status(lambda: b.state_moments()) == 5
        b.set_labels(np.zeros(n, dtype=np.int64))
        assert b.state_hist(24).sum() == n * S
        for shift in (-8, 4, 12, 32):
            assert status(lambda: b.state_hist(shift, np.zeros((K, S, 1), dtype=np.uint32))) == 1
        for J in (0, 17):
            assert status(lambda: b.state_hist(8, np.zeros((K, S, J), dtype=np.uint32))) == 1
        assert status(lambda: b.state_hist(24, np.zeros((K, S, 2), dtype=np.uint32))) == 1
        assert status(lambda: b.state_moments(0, want_bands=True)) == 5       # bands without a grid
        assert b.state_moments()[0].tolist() == [n, 0, 0]
    finally:
        b.close()


# ---- end to end --------------------------------------------------------------------------------------------------------
def _model(K, params):
    from phylo_hmrf_amd import model_io, synthetic
    from phylo_hmrf_amd.tree import PhyloTree
    tree = PhyloTree(synthetic.tree_for(4))
    means, covars = tree.mean_cov(params, 2e-3)
    return model_io.Model(K=K, S=4, edge_list=np.asarray(synthetic.tree_for(4), dtype=np.int64), branch_list=None, species=None,
                          means_=means, _covars_=covars, params_vec=np.asarray(params), params_vec1=np.asarray(params),
                          min_covar=2e-3, beta=1.0, beta1=0.5, estimate_type=0, num_neighbor=8, energy_tol_ppb=10000,
                          x_max=float("nan"), resolution=-1, filter_mode=-1, filter_sigma=float("nan"), diagonal_type=-1,
                          tree=tree)


def _check_profile(prof, ref, K, quantiles):
    for k in ("count", "count_region", "bands"):
        assert np.array_equal(prof[k], ref[k]), k
    for k in ("q_lo", "q_hi"):
        assert prof[k].dtype == np.float32
        assert np.array_equal(prof[k].view(np.uint32), ref[k].view(np.uint32)), k
    scale = np.maximum(np.abs(ref["q_lo"]), np.abs(ref["q_hi"])).astype(np.float64)
    assert np.all(np.abs(prof["q"] - ref["q"]) <= 4 * 2.0 ** -52 * scale)
    n = ref["count"].astype(np.float64)[:, None]
    slack = np.maximum(n - 1, 0) * 2.0 ** -53
    # mean = sum / n: the sum's bound over n, and one more rounding of the quotient
    assert np.all(np.abs(prof["mean"] - ref["sum"] / n) <= slack * ref["abs_sum"] / n + 2.0 ** -52 * np.abs(ref["sum"] / n))
    mean, sd = P.moments(ref["count"], ref["sum"], ref["sumsq"])
    assert np.allclose(prof["sd"], sd, rtol=1e-9, atol=0)
    assert np.array_equal(prof["share"], ref["count"] / float(ref["count"].sum()))
    med = prof["q"][:, :, list(quantiles).index(0.5)]
    assert np.array_equal(prof["order"], P.state_order(ref["count"], med))
    assert prof["chrom"].tolist() == [1] and prof["enrichment"].shape == (1, K)
    assert np.allclose(prof["enrichment"], np.log2(1.0 + 1e-16), atol=1e-12)


def test_state_profile_end_to_end_after_segment():
    from phylo_hmrf_amd.hmrf import phyloHMRF
    N, K = 48, 3
    blk = synth.make_block(seed=4, H=N, W=N, S=4, K=K, diagonal=True)
    X = blk["X"]
    n = X.shape[0]
    len_vec = [[n, 0, n, N, N, 0, 0, 0, 1, 1]]
    m = phyloHMRF.from_model(_model(K, blk["params"]), X, len_vec, [blk["edges"]], quiet=True)
    try:
        labels = m.segment()["state_vec"].astype(np.int64)
        assert len(np.unique(labels)) == K
        prof = m.state_profile()
        x32 = X.astype(np.float32)
        _check_profile(prof, SR.state_profile(x32, labels, len_vec, K, P.DEFAULT_QUANTILES), K, P.DEFAULT_QUANTILES)
        assert [p["shift"] for p in prof["timing"]["passes"]] == [24, 16, 8, 0] and prof["timing"]["total"] > 0
        # a permuted labelling, uploaded as state_vec, permutes the rows
        perm = np.array([2, 0, 1])
        other = m.state_profile(state_vec=perm[labels].astype(np.float64))
        for k in ("count", "mean", "sd", "q_lo", "q_hi", "q", "bands", "share"):
            assert np.array_equal(other[k][perm], prof[k], equal_nan=True), k
        assert np.array_equal(other["count_region"][:, perm], prof["count_region"])
        _check_profile(other, SR.state_profile(x32, perm[labels], len_vec, K, P.DEFAULT_QUANTILES), K, P.DEFAULT_QUANTILES)
        # other quantiles, none of them the median: `order` still comes from the medians
        few = m.state_profile(quantiles=(0.1, 1.0), want_bands=False)
        assert few["bands"] is None and np.array_equal(few["order"], other["order"])
        assert np.array_equal(few["q_hi"][:, :, 1], np.stack([[x32[perm[labels] == k, s].max() for s in range(4)] for k in range(K)]))
    finally:
        m.close()


def test_cli_profile_after_a_fit(tmp_path):
    """--profile 1 with a fit: the state_vec of the .mat is what profile_<run_id>_<K>.npz and .txt describe"""
    import scipy.io
    import phylo_hmrf as cli
    out = str(tmp_path / "fit")
    f = cli.run("4", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", out, synthetic="48", seed="5",
                quiet="1", profile="1", profile_quantiles="0.25,0.5,0.75")
    state_vec = scipy.io.loadmat(f)["state_vec"].reshape(-1).astype(np.int64)
    prof = P.load_npz(out + "/profile_0_4.npz")
    assert np.array_equal(prof["count"], np.bincount(state_vec, minlength=4))
    assert prof["quantiles"].tolist() == [0.25, 0.5, 0.75] and prof["q"].shape == (4, 4, 3)
    assert prof["bands"].sum() == state_vec.size == 48 * 49 // 2
    lines = open(out + "/profile_0_4.txt").read().splitlines()
    assert len(lines) == 1 + 4 * 4 and lines[1].split("\t")[:3] == ["1", "species1", str(prof["count"][0])]
