"""GPU: the post-processing's small-region smoothing (phmrf_smooth_labels through smooth.smooth_states) against the
full-matrix restatement of tests/smooth_reference.py, exactly, on the reference's chr22 labelling, noisy synthetic maps of
diagonal and off-diagonal blocks of many shapes and state counts; repeatability, refused input, and the command line from a
fit to the written files."""
import ctypes
import os

import numpy as np
import pytest

from tests import smooth_reference as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _noisy_map(seed, H, W, K, p=0.1, mean_run=25):
    """synthetic.label_image with salt-and-pepper noise: a share p of the bins takes a uniformly drawn state"""
    from phylo_hmrf_amd import synthetic
    rng = np.random.default_rng(seed)
    img = synthetic.label_image(rng, H, W, K, mean_run)
    noise = rng.random((H, W)) < p
    img[noise] = rng.integers(0, K, int(noise.sum()))
    return img


def _region(seed, H, W, diagonal, K, p=0.1):
    img = _noisy_map(seed, H, W, K, p)
    sv = S.upper_nodes(img, diagonal).astype(np.int64)
    n = sv.shape[0]
    return sv, np.array([[n, 0, n, H, W, 0, 0, 0, 1 if diagonal else 0, 1]])


def _check(sv, lv, **kw):
    from phylo_hmrf_amd.smooth import smooth_states
    got, counts = smooth_states(sv, lv, **kw)
    want = S.smooth_state_vec(sv, lv, **kw)
    assert got.dtype == sv.dtype and got.shape == sv.shape
    assert np.array_equal(got, want), int((got != want).sum())
    return got, counts


@pytest.fixture(scope="module")
def chr22():
    g = np.load(os.path.join(G, "example_chr22_full.npz"))
    return g["it_labels"][-1].astype(np.int64), g["len_vec"]


@pytest.mark.parametrize("window", [3, 5, 7])
@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("max_area", [None, 0, 10 ** 9])
def test_chr22_labelling_equals_the_restatement(chr22, window, n_iter, max_area):
    sv, lv = chr22
    got, counts = _check(sv, lv, window=window, max_area=max_area, n_iter=n_iter)
    assert counts.shape == (1, n_iter, 3)
    if n_iter == 1:
        assert counts[0, 0, 2] == int((got != sv).sum())
    if max_area == 0:
        assert not counts.any() and np.array_equal(got, sv)
    if (window, n_iter, max_area) == (5, 1, None):
        print("chr22 at the defaults: %d small components, %d relabelled, %d of %d nodes changed"
              % (counts[0, 0, 0], counts[0, 0, 1], counts[0, 0, 2], sv.shape[0]))


@pytest.mark.parametrize("N", [1, 2, 3, 5, 64, 257, 2000])
def test_noisy_diagonal_blocks(N):
    sv, lv = _region(N, N, N, True, 20)
    _check(sv, lv)
    _check(sv, lv, window=3, max_area=10 ** 9, n_iter=2)


@pytest.mark.parametrize("H,W", [(37, 91), (1, 50), (50, 1)])
def test_noisy_off_diagonal_blocks(H, W):
    sv, lv = _region(H * 1000 + W, H, W, False, 20, p=0.2)
    _check(sv, lv)
    _check(sv, lv, window=3, max_area=10 ** 9)
    _check(sv, lv, window=4, max_area=40, n_iter=3)


@pytest.mark.parametrize("K", [2, 7, 20, 64])
def test_state_counts(K):
    a, _ = _region(K, 150, 150, True, K, p=0.3)
    b, _ = _region(K + 1, 40, 70, False, K, p=0.3)
    sv = np.concatenate([a, b])
    lv = np.array([[a.size, 0, a.size, 150, 150, 0, 0, 0, 1, 1],
                   [b.size, a.size, a.size + b.size, 40, 70, 0, 150, 1, 0, 1]])
    _check(sv, lv)
    _check(sv, lv, window=5, max_area=200, n_iter=2)


def test_two_runs_are_identical_and_shapes_dtypes_are_kept(chr22):
    from phylo_hmrf_amd.smooth import smooth_states
    sv, lv = chr22
    a, ca = smooth_states(sv.astype(np.uint8).reshape(1, -1), lv, window=7, max_area=10 ** 9, n_iter=3)
    b, cb = smooth_states(sv.astype(np.uint8).reshape(1, -1), lv, window=7, max_area=10 ** 9, n_iter=3)
    assert a.dtype == np.uint8 and a.shape == (1, sv.size)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    c, _ = smooth_states(sv.astype(np.float64), lv, window=7, max_area=10 ** 9, n_iter=3)
    assert c.dtype == np.float64 and np.array_equal(c.astype(np.uint8), a.reshape(-1))


def test_device_entry_refuses_bad_input_and_works_in_place():
    import torch
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    sv, _ = _region(3, 30, 30, True, 6, p=0.3)
    dev = torch.device("cuda", 0)
    src = torch.from_numpy(sv.astype(np.uint8)).to(dev)
    out = torch.full_like(src, 77)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    cnt = np.zeros(3, dtype=np.int64)

    def call(K, window=5, H=30, W=30, diag=1, dst=out):
        return L.phmrf_smooth_labels(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), H, W, diag, K,
                                     window, 25, 1, _lib.ptr_i64(cnt), st)

    assert call(5) == 1                                     # a label >= K: PHMRF_ERR_INVALID, nothing written
    assert int((out == 77).sum()) == out.numel()
    assert call(65) == 4                                    # K > 64: PHMRF_ERR_UNSUPPORTED
    assert call(6, window=0) == 1
    assert call(6, W=29) == 1                               # a non-square diagonal block
    assert int((out == 77).sum()) == out.numel()
    assert call(6) == 0
    want = S.smooth_region(sv, 30, 30, True, window=5, max_area=25)
    assert np.array_equal(out.cpu().numpy(), want.astype(np.uint8))
    assert call(6, dst=src) == 0                            # in place
    assert np.array_equal(src.cpu().numpy(), want.astype(np.uint8))


def _cli(out, extra, seed=5):
    import phylo_hmrf as cli
    return cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", out, synthetic="64",
                   seed=str(seed), quiet="1", **extra)


def test_cli_fit_then_postprocess(tmp_path):
    import scipy.io
    from phylo_hmrf_amd.smooth import smooth_states
    fit_dir, pp_dir = str(tmp_path / "fit"), str(tmp_path / "pp")
    f = _cli(fit_dir, {})
    assert os.path.basename(f) == "estimate_ou_0_1.00_5.mat"
    out = _cli(pp_dir, dict(postprocess=f, smooth_window="3", smooth_area="-1", smooth_iter="2"))
    assert os.path.basename(out) == "smooth_estimate_ou_0_1.00_5.mat"
    d = scipy.io.loadmat(out)
    fit = scipy.io.loadmat(f)
    sv = fit["state_vec"].reshape(-1)
    n = 64 * 65 // 2
    assert sv.size == n and np.array_equal(d["state_vec"].reshape(-1), sv)
    want, counts = smooth_states(sv, fit["len_vec"], window=3, n_iter=2)
    assert np.array_equal(d["state_vec_smooth"].reshape(-1), want)
    assert np.array_equal(d["smooth_counts"].reshape(counts.shape), counts)
    assert [int(np.ravel(d[k])[0]) for k in ("smooth_window", "smooth_iter", "smooth_area")] == [3, 2, 25]
    for annot, states in (("ori", sv), ("smooth", want)):
        lines = open(os.path.join(pp_dir, "estimate_test1.%s.txt" % annot), "rb").read().split(b"\r\n")
        assert lines[-1] == b"" and len(lines) - 1 == n
        cols = np.array([[int(x) for x in ln.split(b"\t")] for ln in lines[:-1]])
        assert np.array_equal(cols[:, 6], states + 1)
        iu = np.triu_indices(64)
        assert np.array_equal(cols[:, 1], iu[0] * 50000) and np.array_equal(cols[:, 4], iu[1] * 50000)
    assert open(os.path.join(pp_dir, "test1.region.txt")).read() == "%d\t1\t%d\t64\t64\t0\t0\n" % (n, n)
