"""GPU: the comparison of two state maps (phmrf_label_contingency, phmrf_diff_domains, phylo_hmrf_amd.compare) against the
full-matrix restatement of tests/compare_reference.py.  Everything is integer arithmetic: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

from tests import compare_reference as C

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def gpu():
    import torch
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    return L, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _put(dev, x, dtype=np.uint8, offset=0):
    """x on the device, `offset` bytes (entries, for float32) past the start of its allocation"""
    import torch
    x = np.ascontiguousarray(np.asarray(x).astype(dtype))
    buf = torch.zeros(x.size + offset + 1, dtype=torch.from_numpy(x[:0]).dtype, device=dev)
    view = buf[offset:offset + x.size]
    view.copy_(torch.from_numpy(x))
    return view


def _contingency(gpu, a, b, KA, KB, off_a=0, off_b=0, fill=0):
    from phylo_hmrf_amd import _lib
    L, dev, st = gpu
    a_t, b_t = _put(dev, a, offset=off_a), _put(dev, b, offset=off_b)
    assert a_t.data_ptr() % 4 == off_a % 4 and b_t.data_ptr() % 4 == off_b % 4
    out = np.full(KA * KB, fill, dtype=np.int64)
    status = L.phmrf_label_contingency(ctypes.c_void_p(a_t.data_ptr()), ctypes.c_void_p(b_t.data_ptr()), len(a), KA, KB,
                                       _lib.ptr_i64(out), st)
    return status, out.reshape(KA, KB)


def _maps(seed, n, KA, KB):
    """three pairs of maps: random, piecewise constant (runs of 1 - 40), and with no two equal neighbours"""
    rng = np.random.default_rng(seed)
    yield rng.integers(0, KA, n), rng.integers(0, KB, n)
    runs = lambda K: np.repeat(rng.integers(0, K, n), rng.integers(1, 41, n))[:n]
    yield runs(KA), runs(KB)
    v = np.arange(n)
    yield (v + seed) % KA, (v // 3 + v) % KB


@pytest.mark.parametrize("KA,KB", [(1, 1), (2, 3), (20, 20), (64, 64), (64, 1)])
def test_contingency_sizes_and_state_counts(gpu, KA, KB):
    for n in (1, 63, 64, 65, 255, 256, 257, 1027):
        for a, b in _maps(n, n, KA, KB):
            status, got = _contingency(gpu, a, b, KA, KB)
            assert status == 0 and np.array_equal(got, C.contingency(a, b, KA, KB)), (n, KA, KB)


@pytest.mark.parametrize("n", [1024 * 256 + 5, 1024 * 1024 + 5, 2 * 1024 * 1024 + 1027])
def test_contingency_past_the_grid_cap(gpu, n):
    """n just above cap x 256 lanes, and just above cap x 1024 nodes (a lane reads four): the second and third trips"""
    from phylo_hmrf_amd import compare
    assert compare.CONTINGENCY_GRID_CAP == 1024 and compare.CONTINGENCY_PER_TRIP == 1024     # (pinned on the source, CPU test)
    for a, b in list(_maps(7, n, 20, 20))[:2]:
        status, got = _contingency(gpu, a, b, 20, 20)
        assert status == 0 and np.array_equal(got, C.contingency(a, b, 20, 20))
        assert got.sum() == n


@pytest.mark.parametrize("off_a,off_b", [(1, 1), (3, 3), (2, 2), (1, 3), (0, 2)])
def test_contingency_of_unaligned_buffers(gpu, off_a, off_b):
    """equal offsets: a byte-wise head, then words; different ones: the maps cannot be aligned together, all byte-wise"""
    for n in (1, 2, 3, 4, 5, 66, 1027, 5000):
        for a, b in _maps(n + off_a, n, 7, 5):
            status, got = _contingency(gpu, a, b, 7, 5, off_a, off_b)
            assert status == 0 and np.array_equal(got, C.contingency(a, b, 7, 5)), (n, off_a, off_b)


def test_contingency_errors_leave_the_output_alone(gpu):
    L, dev, st = gpu
    a = np.zeros(1000, dtype=np.int64)
    b = a.copy()
    for where in (0, 1, 2, 3, 500, 997, 998, 999):          # a word's every byte, the tail
        for which in (0, 1):
            x, y = a.copy(), b.copy()
            (x, y)[which][where] = 5
            status, got = _contingency(gpu, x, y, 5, 5, 1, 1, fill=77)
            assert status == INVALID and (got == 77).all(), (where, which)
    assert _contingency(gpu, a, b, 65, 2, fill=77)[0] == UNSUPPORTED
    assert _contingency(gpu, a, b, 2, 0, fill=77)[0] == INVALID
    from phylo_hmrf_amd import _lib
    out = np.full(4, 77, dtype=np.int64)
    a_t = _put(dev, a)
    p = ctypes.c_void_p(a_t.data_ptr())
    assert L.phmrf_label_contingency(p, None, 1000, 2, 2, _lib.ptr_i64(out), st) == INVALID
    assert L.phmrf_label_contingency(p, p, -1, 2, 2, _lib.ptr_i64(out), st) == INVALID
    assert L.phmrf_label_contingency(p, p, 1000, 2, 2, None, st) == INVALID
    assert L.phmrf_label_contingency(p, p, 2 ** 31 - 64, 2, 2, _lib.ptr_i64(out), st) == UNSUPPORTED
    assert (out == 77).all()
    assert L.phmrf_label_contingency(p, p, 0, 2, 2, _lib.ptr_i64(out), st) == 0 and not out.any()


# ---- differential domains ---------------------------------------------------------------------------------------------------
def _domains(gpu, a, b, H, W, diag, dist0=0, KA=None, KB=None, min_area=1, map_b=None, conf_a=None, conf_b=None, min_conf=0.0,
             capacity=None, want_diff=True, want_bands=True):
    """-> (status, diff, table rows written, n_domains, bands, the whole table buffer)"""
    from phylo_hmrf_amd import _lib
    L, dev, st = gpu
    n = len(a)
    KA = int(np.max(a)) + 1 if KA is None else KA
    KB = int(np.max(b)) + 1 if KB is None else KB
    a_t, b_t = _put(dev, a), _put(dev, b)
    ca_t = None if conf_a is None else _put(dev, conf_a, np.float32)
    cb_t = None if conf_b is None else _put(dev, conf_b, np.float32)
    diff_t = _put(dev, np.full(n, 9))
    capacity = n if capacity is None else capacity
    table = np.full((max(capacity, 1), 12), -7, dtype=np.int64)
    bands = np.full((32, 3), -7, dtype=np.int64)
    found = ctypes.c_int64(-7)
    m = None if map_b is None else np.ascontiguousarray(np.asarray(map_b, dtype=np.uint8))
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    status = L.phmrf_diff_domains(ptr(a_t), ptr(b_t), None if m is None else m.ctypes.data_as(ctypes.c_void_p), ptr(ca_t),
                                  ptr(cb_t), H, W, int(diag), dist0, KA, KB, min_conf, min_area,
                                  ptr(diff_t) if want_diff else None, capacity, _lib.ptr_i64(table), ctypes.byref(found),
                                  _lib.ptr_i64(bands) if want_bands else None, st)
    k = max(0, min(int(found.value), capacity))
    return status, diff_t.cpu().numpy(), table[:k], int(found.value), bands, table


def _blocky(rng, H, W, K):
    """a piecewise-constant map: constant tiles of 1 - 9 rows by 1 - 9 columns"""
    rows = np.repeat(np.arange(H), rng.integers(1, 10, H))[:H]
    cols = np.repeat(np.arange(W), rng.integers(1, 10, W))[:W]
    return rng.integers(0, K, (H, W))[rows][:, cols]


def _pair(seed, H, W, diag, K=6):
    """A blocky; B = A with seeded rectangles and single pixels relabelled; two confidences on both sides of 0.5"""
    rng = np.random.default_rng(seed)
    A = _blocky(rng, H, W, K)
    B = A.copy()
    for _ in range(6):
        i, j = rng.integers(0, H), rng.integers(0, W)
        h, w = rng.integers(1, max(2, H // 3 + 1)), rng.integers(1, max(2, W // 3 + 1))
        B[i:i + h, j:j + w] = (B[i:i + h, j:j + w] + rng.integers(1, K)) % K
    for _ in range(max(1, H * W // 40)):
        i, j = rng.integers(0, H), rng.integers(0, W)
        B[i, j] = (B[i, j] + 1) % K
    pick = (lambda M: M[np.triu_indices(H)]) if diag else (lambda M: M.reshape(-1))
    a, b = pick(A), pick(B)
    conf = lambda: np.where(rng.random(a.size) < 0.3, rng.random(a.size) * 0.5, 0.5 + rng.random(a.size) * 0.5).astype(np.float32)
    ca, cb = conf(), conf()
    ca[::7] = 0.5                                            # exactly on the threshold: counts
    ca[::11], cb[::13] = 0.0, 1.0
    return a, b, ca, cb


def _check(gpu, a, b, H, W, diag, dist0=0, **kw):
    status, diff, table, found, bands, _ = _domains(gpu, a, b, H, W, diag, dist0, **kw)
    assert status == 0
    ref = dict((k, v) for k, v in kw.items() if k in ("min_area", "map_b", "conf_a", "conf_b", "min_conf"))
    want_diff, want_table, want_bands = C.compare_region(a, b, H, W, diag, dist0, **ref)
    assert np.array_equal(diff, want_diff)
    assert found == want_table.shape[0], (found, want_table.shape[0])
    assert np.array_equal(table, want_table), (table.tolist(), want_table.tolist())
    assert np.array_equal(bands, want_bands)
    return table


def _all_options(gpu, a, b, ca, cb, H, W, diag, dist0, K=6):
    rng = np.random.default_rng(H * 131 + W)
    perm = rng.permutation(K)
    for map_b in (None, perm, np.minimum(perm + 3, 63)):
        for min_area in (1, 5):
            _check(gpu, a, b, H, W, diag, dist0, KA=K, KB=K, min_area=min_area, map_b=map_b)
            for min_conf in (0.0, 0.5):
                _check(gpu, a, b, H, W, diag, dist0, KA=K, KB=K, min_area=min_area, map_b=map_b, conf_a=ca, conf_b=cb,
                       min_conf=min_conf)


@pytest.mark.parametrize("H", [1, 2, 3, 17, 64, 65, 130])
def test_domains_of_diagonal_blocks(gpu, H):
    a, b, ca, cb = _pair(H, H, H, True)
    _all_options(gpu, a, b, ca, cb, H, H, True, 0)


@pytest.mark.parametrize("H,W,dist0", [(1, 12, 3), (12, 1, 40), (7, 10, -4), (40, 70, 1000), (40, 70, -30)])
def test_domains_of_off_diagonal_blocks(gpu, H, W, dist0):
    a, b, ca, cb = _pair(H * 100 + W, H, W, False)
    _all_options(gpu, a, b, ca, cb, H, W, False, dist0)


@pytest.mark.parametrize("H,W,diag", [(65, 65, True), (40, 70, False), (300, 300, True)])
def test_equal_maps_opposite_maps_and_the_most_domains(gpu, H, W, diag):
    a, _, ca, cb = _pair(5, H, W, diag)
    n = a.size
    t = _check(gpu, a, a, H, W, diag, 7 * (not diag), KA=6, KB=6)               # B == A: nothing
    assert t.shape == (0, 12)
    t = _check(gpu, a, (a + 1) % 6, H, W, diag, 7 * (not diag), KA=6, KB=6, conf_a=ca, conf_b=cb)   # different everywhere
    assert t.shape == (1, 12) and t[0, 0] == 0 and t[0, 5] == n and t[0, 6] == (H * H if diag else n)
    ii, jj = C.node_coords(H, W, diag)
    lattice = (ii % 2 == 0) & (jj % 2 == 0)                  # isolated pixels: as many domains as a map can have
    b = np.where(lattice, (a + 1) % 6, a)
    t = _check(gpu, a, b, H, W, diag, 7 * (not diag), KA=6, KB=6, conf_a=ca, conf_b=cb)
    assert t.shape[0] == int(lattice.sum()) and (t[:, 6] == 1).all() and np.array_equal(t[:, 0], np.nonzero(lattice)[0])
    assert _check(gpu, a, b, H, W, diag, 7 * (not diag), KA=6, KB=6, min_area=2).shape == (0, 12)


def test_domains_of_a_block_past_the_grid_cap(gpu):
    """1.1 M nodes: every kernel's grid is capped and strides, a workgroup of the compaction owns more than 256 nodes"""
    H = 1500
    a, b, ca, cb = _pair(77, H, H, True)
    assert a.size > 4096 * 256
    t = _check(gpu, a, b, H, H, True, KA=6, KB=6, conf_a=ca, conf_b=cb, min_conf=0.5)
    assert t.shape[0] > 4096


def test_capacity_zero_and_a_capacity_below_the_count(gpu):
    a, b, ca, cb = _pair(11, 65, 65, True)
    _, full, bands0 = C.compare_region(a, b, 65, 65, True, conf_a=ca, conf_b=cb)
    D = full.shape[0]
    assert D > 8
    status, _, rows, found, bands, buf = _domains(gpu, a, b, 65, 65, True, capacity=0, conf_a=ca, conf_b=cb)
    assert status == 0 and found == D and (buf == -7).all() and np.array_equal(bands, bands0)
    L, dev, st = gpu
    for cap in (1, 5, D - 1, D, D + 3):
        status, _, rows, found, _, buf = _domains(gpu, a, b, 65, 65, True, capacity=cap, conf_a=ca, conf_b=cb)
        assert status == 0 and found == D
        assert np.array_equal(rows, full[:cap]) and (buf[min(cap, D):] == -7).all()
    # no diff map, no bands asked for
    status, diff, rows, found, bands, _ = _domains(gpu, a, b, 65, 65, True, want_diff=False, want_bands=False)
    assert status == 0 and found == D and (diff == 9).all() and (bands == -7).all()


def test_two_calls_give_the_same_bytes(gpu):
    a, b, ca, cb = _pair(3, 130, 130, True)
    one = _domains(gpu, a, b, 130, 130, True, conf_a=ca, conf_b=cb, min_conf=0.5)
    two = _domains(gpu, a, b, 130, 130, True, conf_a=ca, conf_b=cb, min_conf=0.5)
    assert one[0] == two[0] == 0 and one[3] == two[3] > 0
    for x, y in zip(one[1:], two[1:]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_domain_error_codes(gpu):
    a, b, ca, cb = _pair(2, 17, 17, True)
    ok = dict(KA=6, KB=6)

    def status(*args, **kw):
        s, diff, _, found, bands, buf = _domains(gpu, *args, **dict(ok, **kw))
        if s != 0:
            assert (diff == 9).all() and found == -7 and (bands == -7).all() and (buf == -7).all()      # nothing written
        return s

    assert status(a, b, 17, 17, True) == 0
    assert status(a, b, 17, 17, True, KA=int(a.max())) == INVALID                 # a label >= K
    assert status(a, b, 17, 17, True, KB=int(b.max())) == INVALID
    assert status(a, b, 17, 17, True, KA=65) == UNSUPPORTED
    assert status(a, b, 17, 17, True, KB=0) == INVALID
    assert status(a, b, 17, 18, True) == INVALID                                  # a non-square diagonal block
    assert status(a, b, 0, 17, False) == INVALID
    assert status(a, b, 17, 17, 2) == INVALID
    assert status(a, b, 17, 17, True, capacity=-1) == INVALID
    assert status(a, b, 17, 17, True, min_area=0) == INVALID
    assert status(a, b, 17, 17, True, conf_a=ca) == INVALID                       # one confidence without the other
    assert status(a, b, 17, 17, True, map_b=[0, 1, 2, 3, 4, 64]) == INVALID
    assert status(a, b, 17, 17, True, dist0=2 ** 31) == INVALID
    for bad in (np.nan, np.inf, -0.25, 1.5):
        for which in (0, 1):
            for where in (0, a.size - 1):                    # at a node that differs or not: every node is checked
                c = [ca.copy(), cb.copy()]
                c[which][where] = bad
                assert status(a, b, 17, 17, True, conf_a=c[0], conf_b=c[1], min_conf=0.5) == INVALID
    from phylo_hmrf_amd import _lib
    L, dev, st = gpu
    a_t = _put(dev, a)
    p = ctypes.c_void_p(a_t.data_ptr())
    found = ctypes.c_int64(0)
    assert L.phmrf_diff_domains(p, p, None, None, None, 17, 17, 1, 0, 6, 6, 0.0, 1, None, 4, None, ctypes.byref(found), None,
                                st) == INVALID                                    # capacity > 0 without a table
    assert L.phmrf_diff_domains(p, None, None, None, None, 17, 17, 1, 0, 6, 6, 0.0, 1, None, 0, None, ctypes.byref(found),
                                None, st) == INVALID
    assert L.phmrf_diff_domains(p, p, None, None, None, 17, 17, 1, 0, 6, 6, 0.0, 1, None, 0, None, None, None, st) == INVALID
    assert L.phmrf_diff_domains(p, p, None, None, None, 17, 17, 1, 0, 6, 6, 0.0, 1, None, 0, None, ctypes.byref(found), None,
                                st) == 0 and found.value == 0


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _two_regions(seed=21, K=6):
    a1, b1, ca1, cb1 = _pair(seed, 130, 130, True, K)
    a2, b2, ca2, cb2 = _pair(seed + 1, 40, 70, False, K)
    n1, n2 = a1.size, a2.size
    lv = np.array([[n1, 0, n1, 130, 130, 10, 10, 0, 1, 3], [n2, n1, n1 + n2, 40, 70, 10, 200, 1, 0, 3]])
    return (np.concatenate([a1, a2]), np.concatenate([b1, b2]), np.concatenate([ca1, ca2]), np.concatenate([cb1, cb2]), lv)


def _check_states(res, a, b, lv, map_b, ca=None, cb=None, min_conf=0.0, min_area=None):
    from phylo_hmrf_amd import compare
    KA, KB = int(a.max()) + 1, int(b.max()) + 1
    raw = np.stack([C.contingency(a[r[1]:r[2]], b[r[1]:r[2]], KA, KB) for r in lv])
    want = compare.permute_columns(raw, map_b)
    assert np.array_equal(res["map_b"], map_b) and res["map_b"].dtype == np.uint8
    assert np.array_equal(res["contingency_region"], want) and np.array_equal(res["contingency"], want.sum(axis=0))
    s = compare.scores(want.sum(axis=0))
    assert (res["agreement"], res["ari"], res["nmi"]) == (s["agreement"], s["ari"], s["nmi"])
    assert np.array_equal(res["agreement_region"], [np.trace(w) / w.sum() for w in want])
    diff, table, bands = C.compare_state_vec(a, b, lv, map_b, ca, cb, min_conf, min_area)
    assert res["diff_vec"].dtype == np.uint8 and np.array_equal(res["diff_vec"], diff)
    assert np.array_equal(res["band_counts"], bands)
    assert res["domains"].dtype == np.int64 and np.array_equal(res["domains"], table)
    if ca is None:
        assert res["domain_conf"].shape == (table.shape[0], 2) and np.isnan(res["domain_conf"]).all()
    else:
        assert np.array_equal(res["domain_conf"], table[:, 10:12] / (table[:, 6:7] * float(1 << 24)))
    return table


def test_compare_states_on_two_regions(monkeypatch):
    from phylo_hmrf_amd import compare
    a, b, ca, cb, lv = _two_regions()
    ident = np.arange(6, dtype=np.uint8)
    t = _check_states(compare.compare_states(a, b, lv, min_area=1), a, b, lv, ident, min_area=1)
    assert t.shape[0] > 4 and set(t[:, 0]) == {0, 1}
    _check_states(compare.compare_states(a, b, lv), a, b, lv, ident)                      # the default area rule: 81 / 26
    _check_states(compare.compare_states(a, b, lv, ca, cb, min_conf=0.5, min_area=3), a, b, lv, ident, ca, cb, 0.5, 3)
    # B with its states renumbered: matching finds the inverse permutation, and everything equals the run before
    perm = np.array([4, 2, 0, 5, 1, 3])
    res = compare.compare_states(a, perm[b], lv, ca, cb, match=True, min_conf=0.5, min_area=3)
    _check_states(res, a, perm[b], lv, np.argsort(perm).astype(np.uint8), ca, cb, 0.5, 3)
    again = compare.compare_states(a, b, lv, ca, cb, min_conf=0.5, min_area=3)
    for k in ("contingency", "contingency_region", "diff_vec", "domains", "band_counts", "domain_conf"):
        assert np.array_equal(res[k], again[k]), k
    # a first call whose table is too small is followed by one of the right size
    monkeypatch.setattr(compare, "FIRST_CAPACITY", 2)
    small = compare.compare_states(a, b, lv, ca, cb, min_conf=0.5, min_area=3)
    assert small["domains"].shape[0] > 4 and np.array_equal(small["domains"], again["domains"])
    # the states of the float64 1 x n layout of a .mat file
    res = compare.compare_states(a.astype(np.float64).reshape(1, -1), b.reshape(1, -1), lv.astype(np.float64), min_area=1)
    _check_states(res, a, b, lv, ident, min_area=1)


def _cli(out, **extra):
    import phylo_hmrf as cli
    return cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "25000", "1", "hg38", out, quiet="1", **extra)


def _scalar(x):
    return np.asarray(x).reshape(-1)[0].item()


def test_cli_compare_writes_the_mat_and_the_domain_list(tmp_path):
    import scipy.io
    a, b, ca, cb, lv = _two_regions(seed=33)
    perm = np.array([4, 2, 0, 5, 1, 3])
    smooth_b = b.copy()
    smooth_b[:50] = a[:50]
    fa, fb = str(tmp_path / "segment_0_6.mat"), str(tmp_path / "other.mat")
    scipy.io.savemat(fa, {"state_vec": a, "state_vec_smooth": a, "len_vec": lv, "conf": ca})
    scipy.io.savemat(fb, {"state_vec": perm[b], "state_vec_smooth": perm[smooth_b], "len_vec": lv, "conf": cb})
    out_dir = str(tmp_path / "out")
    inv = np.argsort(perm).astype(np.uint8)
    for field, bb in (("state_vec", b), ("state_vec_smooth", smooth_b)):
        out = _cli(out_dir, compare=fa, compare_with=fb, compare_field=field, compare_match="1", compare_min_conf="0.5",
                   compare_area="3")
        assert os.path.basename(out) == "compare_segment_0_6__other.mat"
        d = scipy.io.loadmat(out)
        res = dict((k, d[k]) for k in ("contingency", "contingency_region", "band_counts", "domains", "domain_conf"))
        res.update(map_b=d["map_b"].reshape(-1), diff_vec=d["diff_vec"].reshape(-1),
                   agreement_region=d["agreement_region"].reshape(-1),
                   agreement=_scalar(d["agreement"]), ari=_scalar(d["ari"]), nmi=_scalar(d["nmi"]))
        table = _check_states(res, a, perm[bb], lv, inv, ca, cb, 0.5, 3)
        assert str(d["compare_field"][0]) == field and _scalar(d["compare_match"]) == 1 and _scalar(d["compare_min_conf"]) == 0.5
        assert d["compare_area"].reshape(-1).tolist() == [3, 3] and _scalar(d["resolution"]) == 25000
        assert np.array_equal(d["len_vec"], lv)
        text = open(os.path.join(out_dir, "compare_domains_segment_0_6__other.txt"), "rb").read()
        assert b"\r" not in text and text.endswith(b"\n")
        lines = text.decode().split("\n")[:-1]
        assert lines[0] == "#chrom\tstart1\tstop1\tstart2\tstop2\tarea\tnodes\tstateA\tstateB\tconfA\tconfB"
        assert len(lines) - 1 == table.shape[0] > 2
        for line, t in zip(lines[1:], table):
            s1, s2 = lv[t[0], 5], lv[t[0], 6]
            mean = t[10:12] / (t[6] * float(1 << 24))
            want = [3, (s1 + t[2]) * 25000, (s1 + t[3] + 1) * 25000, (s2 + t[4]) * 25000, (s2 + t[5] + 1) * 25000, t[7], t[6],
                    t[8] + 1, t[9] + 1]
            assert line == "\t".join(["%d" % x for x in want] + ["%.6f" % m for m in mean])
    # without --compare_min_conf the confidences still give the means; files without conf give nan
    scipy.io.savemat(fb, {"state_vec": b, "len_vec": lv})
    out = _cli(out_dir, compare=fa, compare_with=fb, compare_area="3")
    d = scipy.io.loadmat(out)
    assert np.isnan(d["domain_conf"]).all() and d["domains"].shape[0] > 2
    lines = open(os.path.join(out_dir, "compare_domains_segment_0_6__other.txt")).read().split("\n")
    assert lines[1].endswith("\tnan\tnan")
