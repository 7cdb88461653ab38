"""GPU: the consensus of several state maps (phmrf_label_consensus, phylo_hmrf_amd.consensus) against the restatement of
tests/consensus_reference.py.  Everything is integer arithmetic: every comparison is exact.  Every output buffer is filled
with a pattern before the call, so that "nothing written" is something a test can see."""
import ctypes

import numpy as np
import pytest

from tests import consensus_reference as R

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4
PLANE, TABLE = 0xEE, -7          # what the device planes and the host tables hold before a call
GUARD = 8                        # bytes of a plane's allocation on either side of the plane


@pytest.fixture(scope="module")
def gpu():
    import torch
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    return L, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _put(dev, x, offset=0):
    """x as uint8 on the device, `offset` bytes past a 4-byte boundary, inside an allocation filled with PLANE"""
    import torch
    x = np.ascontiguousarray(np.asarray(x).astype(np.uint8))
    buf = torch.full((x.size + 2 * GUARD,), PLANE, dtype=torch.uint8, device=dev)
    view = buf[GUARD + offset:GUARD + offset + x.size]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 4 == offset % 4
    return buf, view


def _nodes(H, W, diag):
    return H * (H + 1) // 2 if diag else H * W


def _call(gpu, maps, K, H, W, diag, dist0=0, min_support=None, renumber=None, offsets=None, out_offset=0, want_support=True,
          want_core=True, M=None, null=()):
    """-> (status, dict of what the call left in every buffer: the planes with their guard bytes, the tables)"""
    from phylo_hmrf_amd import _lib
    L, dev, st = gpu
    n = _nodes(H, W, diag)
    M_real = len(maps)
    M = M_real if M is None else M
    offsets = [0] * M_real if offsets is None else offsets
    held = [_put(dev, m, o) for m, o in zip(maps, offsets)]
    ptrs = (ctypes.c_void_p * max(M_real, 1))(*[v.data_ptr() for _, v in held])
    ms = M // 2 + 1 if min_support is None else min_support
    ren = None if renumber is None else np.ascontiguousarray(np.asarray(renumber, dtype=np.uint8))
    planes = dict((k, _put(dev, np.full(n, PLANE), out_offset)) for k in ("consensus", "support", "core"))
    Kt, Mt = max(min(K, 64), 1), max(min(M, 16), 1)
    tabs = dict(support_hist=np.full((Kt, Mt + 1), TABLE, dtype=np.int64), agree=np.full((Mt, Kt, Kt), TABLE, dtype=np.int64),
                pair=np.full((Mt, Mt), TABLE, dtype=np.int64), bands=np.full((32, 3), TABLE, dtype=np.int64))
    plane = lambda k, want: ctypes.c_void_p(planes[k][1].data_ptr()) if want and k not in null else None
    table = lambda k: None if k in null else _lib.ptr_i64(tabs[k])
    status = L.phmrf_label_consensus(
        None if "labels" in null else ctypes.cast(ptrs, ctypes.c_void_p), M, None if ren is None else ren.ctypes.data_as(ctypes.c_void_p),
        K, H, W, int(diag), dist0, ms, plane("consensus", True), plane("support", want_support), plane("core", want_core),
        table("support_hist"), table("agree"), table("pair"), table("bands"), st)
    got = dict(tabs)
    for k, (buf, _) in planes.items():
        got[k] = buf.cpu().numpy()
    got["off"] = out_offset
    return status, got


def _plane(got, k, n):
    lo = GUARD + got["off"]
    whole = got[k]
    assert (whole[:lo] == PLANE).all() and (whole[lo + n:] == PLANE).all(), "%s: a byte outside the plane was written" % k
    return whole[lo:lo + n]


def _untouched(got):
    return all((got[k] == PLANE).all() for k in ("consensus", "support", "core")) and \
        all((got[k] == TABLE).all() for k in ("support_hist", "agree", "pair", "bands"))


def _check(gpu, maps, K, H, W, diag, dist0=0, min_support=None, renumber=None, want_support=True, want_core=True, **kw):
    n = _nodes(H, W, diag)
    want_core = want_core and K < 64
    status, got = _call(gpu, maps, K, H, W, diag, dist0, min_support, renumber, want_support=want_support, want_core=want_core,
                        **kw)
    what = (len(maps), K, H, W, diag, dist0, min_support, kw)
    assert status == 0, what
    ref = R.consensus_region(maps, K, H, W, diag, dist0, min_support, renumber)
    assert np.array_equal(_plane(got, "consensus", n), ref["consensus"]), what
    assert np.array_equal(_plane(got, "support", n), ref["support"] if want_support else np.full(n, PLANE)), what
    assert np.array_equal(_plane(got, "core", n), ref["core"] if want_core else np.full(n, PLANE)), what
    for k in ("support_hist", "agree", "pair", "bands"):
        assert np.array_equal(got[k], ref[k]), (k, what)
    return got


def _kinds(seed, M, n, K):
    """five sets of M maps: random, blocky (runs of 1 - 40 nodes), all equal, all constant and distinct (every node a tie, as far
    as K allows), and noisy copies of one blocky map"""
    rng = np.random.default_rng(seed)
    runs = lambda: np.repeat(rng.integers(0, K, n), rng.integers(1, 41, n))[:n]
    yield "random", [rng.integers(0, K, n) for _ in range(M)]
    yield "blocky", [runs() for _ in range(M)]
    one = runs()
    yield "equal", [one.copy() for _ in range(M)]
    yield "constants", [np.full(n, (m + seed) % K) for m in range(M)]
    noisy = []
    for _ in range(M):
        m = one.copy()
        hit = rng.random(n) < 0.15
        m[hit] = rng.integers(0, K, int(hit.sum()))
        noisy.append(m)
    yield "noisy", noisy


# ---- against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1025])
def test_node_counts(gpu, n):
    for M, K in ((1, 3), (3, 5), (4, 20)):
        for kind, maps in _kinds(n, M, n, K):
            _check(gpu, maps, K, 1, n, False)


def test_second_grid_stride_trip(gpu):
    from phylo_hmrf_amd import consensus
    n = consensus.CONSENSUS_GRID_CAP * consensus.CONSENSUS_PER_TRIP + 7
    rng = np.random.default_rng(2)
    one = np.repeat(rng.integers(0, 4, n // 8 + 1), rng.integers(1, 17, n // 8 + 1))[:n]
    assert one.size == n
    maps = []
    for _ in range(3):
        m = one.copy()
        hit = rng.random(n) < 0.2
        m[hit] = rng.integers(0, 4, int(hit.sum()))
        maps.append(m)
    got = _check(gpu, maps, 4, 1, n, False, dist0=-5, offsets=[1, 0, 3], out_offset=2)
    assert got["support_hist"].sum() == n and got["bands"][:, 0].sum() == n


@pytest.mark.parametrize("H,W,diag", [(1, 1, True), (2, 2, True), (5, 5, True), (65, 65, True), (130, 130, True), (1, 7, False),
                                      (7, 1, False), (63, 65, False)])
def test_block_shapes_and_distances(gpu, H, W, diag):
    n = _nodes(H, W, diag)
    for dist0 in ((0,) if diag else (0, 40, -3, -100000)):
        for kind, maps in _kinds(H + dist0 % 7, 3, n, 6):
            _check(gpu, maps, 6, H, W, diag, dist0=dist0)
    if diag:                                                # the second arm of a split chromosome: a diagonal block off the diagonal
        for kind, maps in _kinds(H, 3, n, 6):
            _check(gpu, maps, 6, H, W, diag, dist0=70)


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 15, 16])
@pytest.mark.parametrize("K", [1, 2, 20, 63, 64])
def test_numbers_of_maps_and_states(gpu, M, K):
    """M = 16, K = 64 and its neighbours take agree in chunks: 8192 // K^2 maps at a time"""
    H, W = 37, 41
    for kind, maps in _kinds(M * 64 + K, M, H * W, K):
        for ms in sorted({1, M // 2 + 1, M}):
            _check(gpu, maps, K, H, W, False, dist0=11, min_support=ms)


def test_chunked_agree_with_a_last_chunk_of_one_map(gpu):
    from phylo_hmrf_amd import consensus
    K = 40                                                  # five maps per chunk: 5 + 5 + 1
    assert consensus.CONSENSUS_AGREE_BINS // (K * K) == 5
    for kind, maps in _kinds(3, 11, 2500, K):
        _check(gpu, maps, K, 50, 50, False, offsets=[m % 4 for m in range(11)], out_offset=1)


def test_every_pair_of_byte_offsets(gpu):
    n = 65
    for oa in range(4):
        for ob in range(4):
            for kind, maps in _kinds(4 * oa + ob, 2, n, 7):
                _check(gpu, maps, 7, 1, n, False, offsets=[oa, ob], out_offset=(oa + 2 * ob) % 4)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 66, 1027, 2051])
def test_mixed_byte_offsets_of_five_maps(gpu, n):
    for offsets in ([0, 1, 2, 3, 0], [3, 3, 1, 0, 2], [1, 1, 1, 1, 1]):
        for kind, maps in _kinds(n, 5, n, 9):
            _check(gpu, maps, 9, 1, n, False, offsets=offsets, out_offset=offsets[1])


def _tables(rng, M, K_raw, K, kind):
    ren = np.full((M, 64), 255, dtype=np.uint8)
    for m in range(M):
        if kind == "permutation":
            ren[m, :K_raw] = rng.permutation(K_raw)
        else:                                               # many raw states to one
            ren[m, :K_raw] = rng.integers(0, K, K_raw)
    return ren


@pytest.mark.parametrize("kind", ["permutation", "many_to_one"])
def test_renumbering(gpu, kind):
    rng = np.random.default_rng(11)
    for M, K_raw, K in ((2, 5, 5), (5, 12, 12), (16, 64, 64), (7, 30, 30)) if kind == "permutation" else \
            ((2, 5, 2), (5, 64, 3), (16, 20, 1), (7, 30, 29)):
        ren = _tables(rng, M, K_raw, K, kind)
        H = 45
        for name, maps in _kinds(M + K, M, _nodes(H, H, True), K_raw):
            _check(gpu, maps, K, H, H, True, renumber=ren, offsets=[(3 * m) % 4 for m in range(M)])


def test_optional_planes(gpu):
    for kind, maps in _kinds(1, 3, 1300, 6):
        _check(gpu, maps, 6, 1, 1300, False, want_support=False)
        _check(gpu, maps, 6, 1, 1300, False, want_core=False)
        _check(gpu, maps, 6, 1, 1300, False, want_support=False, want_core=False, out_offset=3)


def test_two_calls_give_the_same_bytes(gpu):
    for kind, maps in _kinds(8, 7, 5000, 20):
        a = _call(gpu, maps, 20, 50, 100, False, dist0=9, offsets=[0, 1, 2, 3, 0, 1, 2])
        b = _call(gpu, maps, 20, 50, 100, False, dist0=9, offsets=[0, 1, 2, 3, 0, 1, 2])
        assert a[0] == b[0] == 0
        for k in ("consensus", "support", "core", "support_hist", "agree", "pair", "bands"):
            assert a[1][k].tobytes() == b[1][k].tobytes(), k


# ---- refused calls ------------------------------------------------------------------------------------------------------------
def test_refused_labels_leave_every_buffer_alone(gpu):
    n, K = 1000, 5
    clean = [np.zeros(n, dtype=np.int64) for _ in range(3)]
    ren = np.full((3, 64), 255, dtype=np.uint8)
    ren[:, :6] = [0, 1, 2, 3, 4, 7]                         # raw 5 renumbers to 7 >= K, raw 6 .. 63 are no states
    for where in (0, 1, 2, 3, 4, 500, 996, 997, 998, 999):  # a head, a word's every byte, the tail
        for which in (0, 2):
            for label, table in ((5, None), (5, ren), (6, ren), (64, None), (64, ren), (255, None)):
                maps = [m.copy() for m in clean]
                maps[which][where] = label
                status, got = _call(gpu, maps, K, 1, n, False, renumber=table, offsets=[1, 0, 2])
                assert status == INVALID and _untouched(got), (where, which, label)
    status, got = _call(gpu, clean, K, 1, n, False, renumber=ren, offsets=[1, 0, 2])
    assert status == 0 and not _plane(got, "consensus", n).any()


def test_refused_arguments_leave_every_buffer_alone(gpu):
    maps = [np.zeros(36, dtype=np.int64) for _ in range(3)]
    ok = dict(K=4, H=6, W=6, diag=False)

    def refused(want, **kw):
        args = dict(ok, **kw)
        status, got = _call(gpu, args.pop("maps", maps), args.pop("K"), args.pop("H"), args.pop("W"), args.pop("diag"), **args)
        assert status == want and _untouched(got), kw

    refused(INVALID, M=0)
    refused(UNSUPPORTED, maps=[maps[0]] * 17)
    refused(INVALID, K=0)
    refused(UNSUPPORTED, K=65)
    refused(INVALID, K=64, maps=[np.zeros(36, dtype=np.int64)] * 3)          # a core plane at K = 64
    refused(INVALID, min_support=0)
    refused(INVALID, min_support=4)
    refused(INVALID, H=4, W=9, diag=True)                   # a diagonal block that is not square (36 nodes all the same)
    refused(INVALID, H=0, W=36)
    refused(INVALID, dist0=2 ** 31)
    for name in ("labels", "consensus", "support_hist", "agree", "pair", "bands"):
        refused(INVALID, null=(name,))
    L, dev, st = gpu
    from phylo_hmrf_amd import _lib
    held = _put(dev, maps[0])
    ptrs = (ctypes.c_void_p * 2)(held[1].data_ptr(), None)   # a NULL map among the pointers
    out = _put(dev, np.full(36, PLANE))
    t = [np.full(s, TABLE, dtype=np.int64) for s in ((4, 3), (2, 4, 4), (2, 2), (32, 3))]
    status = L.phmrf_label_consensus(ctypes.cast(ptrs, ctypes.c_void_p), 2, None, 4, 6, 6, 0, 0, 1,
                                     ctypes.c_void_p(out[1].data_ptr()), None, None, *[_lib.ptr_i64(x) for x in t], st)
    assert status == INVALID and (out[0].cpu().numpy() == PLANE).all() and all((x == TABLE).all() for x in t)
    assert b"NULL" in L.phmrf_last_error()
    # K = 64 without a core plane is a call like any other
    _check(gpu, [np.full(36, 63), np.full(36, 63), np.zeros(36, dtype=np.int64)], 64, 6, 6, False)


# ---- the module ---------------------------------------------------------------------------------------------------------------
def _blocky_vec(rng, L, K, cell=8):
    """a state_vec whose regions are made of cell x cell blocks of one state"""
    parts = []
    for row in L:
        H, W, diag = int(row[3]), int(row[4]), int(row[8])
        img = np.kron(rng.integers(0, K, ((H + cell - 1) // cell, (W + cell - 1) // cell)), np.ones((cell, cell), dtype=np.int64))
        img = img[:H, :W]
        if diag:
            img = np.triu(img) + np.triu(img, 1).T
        parts.append(img[np.triu_indices(H)] if diag else img.reshape(-1))
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def ensemble():
    """two regions (a diagonal block of 48 bins, the 48 x 40 block beside it), a blocky truth at K = 5 and five copies, each
    under its own permutation of the states and with 10 % of its nodes redrawn"""
    rng = np.random.default_rng(21)
    n1, n2 = 48 * 49 // 2, 48 * 40
    L = np.array([[n1, 0, n1, 48, 48, 0, 0, 0, 1, 1], [n2, n1, n1 + n2, 48, 40, 0, 60, 1, 0, 1]], dtype=np.int64)
    K = 5
    truth = _blocky_vec(rng, L, K)
    assert np.bincount(truth, minlength=K).min() > 0
    perms, copies = [], []
    for m in range(5):
        perms.append(rng.permutation(K))
        noisy = truth.copy()
        hit = rng.random(truth.size) < 0.1
        noisy[hit] = rng.integers(0, K, int(hit.sum()))
        copies.append(perms[m][noisy])                      # state k of the truth is state perms[m][k] of copy m
    return L, K, truth, perms, copies


def test_consensus_states_end_to_end(gpu, ensemble):
    from phylo_hmrf_amd import compare, consensus
    L, K, truth, perms, copies = ensemble
    # copy m's state perms[m][k] is the truth's state k: the inverse permutation brings it back, and perms[0] takes it on to
    # copy 0's numbers, which are the consensus'
    back = [perms[0][np.argsort(p)] for p in perms]
    assert np.array_equal(back[0], np.arange(K))
    for m in range(1, 5):                                   # (on the CPU) the matching recovers every permutation
        C = R.tables(copies[0], np.zeros_like(copies[0]), np.stack([copies[m]]), K)[1][0]
        assert np.array_equal(compare.match_states(C), back[m]), m
    ren = np.full((5, 64), 255, dtype=np.uint8)
    for m in range(5):
        ren[m, :K] = back[m]
    res = consensus.consensus_states(copies, L, match=True)
    ref = R.consensus_state_vec(copies, L, K, renumber=ren)
    assert res["K"] == K and res["M"] == 5 and res["min_support"] == 3
    for k in ("state_vec", "support", "conf", "core_vec", "renumber", "support_hist", "support_hist_region", "agree", "pair",
              "pair_agreement", "band_counts"):
        assert np.array_equal(res[k], ref[k]), k
        assert res[k].dtype == ref[k].dtype, k
    want = consensus.map_scores(ref["agree"])
    for k in ("agreement", "ari", "nmi"):
        assert np.array_equal(res[k], want[k]), k
    # every map is at least as close to the consensus as to any other single map
    for m in range(5):
        for o in range(5):
            if o != m:
                assert res["agreement"][m] >= res["pair_agreement"][m][o], (m, o)
    assert (res["state_vec"] == perms[0][truth]).mean() > 0.98
    # without matching the permuted copies are five unrelated maps: the same call, the identity table
    plain = consensus.consensus_states(copies, L, min_support=5, K=7)
    ref = R.consensus_state_vec(copies, L, 7, min_support=5)
    for k in ("state_vec", "support", "core_vec", "renumber", "support_hist", "agree", "pair", "band_counts"):
        assert np.array_equal(plain[k], ref[k]), k
    with pytest.raises(ValueError, match="K = 4"):
        consensus.consensus_states(copies, L, K=4)
    with pytest.raises(ValueError, match="outside"):
        consensus.consensus_states(copies, L, min_support=6)


def test_consensus_files_and_the_readers_of_its_mat(gpu, ensemble, tmp_path):
    import scipy.io
    from phylo_hmrf_amd import consensus, domains, maps
    L, K, truth, perms, copies = ensemble
    paths = []
    for m, c in enumerate(copies):
        paths.append(str(tmp_path / ("rep%d.mat" % m)))
        scipy.io.savemat(paths[-1], dict(state_vec=c, len_vec=L))
    out_dir = str(tmp_path / "out")
    out = consensus.consensus_files(paths, out_dir, 50000, match=True, min_support=4, min_area=3)
    assert out == str(tmp_path / "out" / "consensus_rep0_5.mat")
    res = consensus.consensus_states(copies, L, match=True, min_support=4)
    s, L2, conf = maps.load_map(out)
    assert np.array_equal(s, res["state_vec"]) and np.array_equal(L2, L) and np.array_equal(conf, res["conf"])
    core, _, _ = maps.load_map(out, "core_vec")
    assert np.array_equal(core, res["core_vec"])
    txt = open(str(tmp_path / "out" / "consensus_rep0_5.txt")).read()
    assert txt == "".join(consensus.summary_lines(res, paths))
    # the domains of core_vec: those of state K are the unstable nodes inside listed areas
    dom = domains.state_domains(core, L, conf, min_area=3)
    listed = open(str(tmp_path / "out" / "consensus_domains_rep0_5.txt")).read()
    assert listed == "".join(domains.domain_lines(dom["domains"], dom["domain_conf"], L, 50000))
    unstable_rows = np.nonzero(dom["domains"][:, 8] == K)[0]
    assert unstable_rows.size > 0 and ("\t%d\t" % (K + 1)) in listed
    in_unstable_domain = np.isin(dom["domain_vec"], unstable_rows)
    in_any_domain = dom["domain_vec"] >= 0
    unstable = res["support"] < 4
    assert np.array_equal(in_unstable_domain, unstable & in_any_domain)
    assert np.array_equal(unstable, core == K)
