"""GPU: the domains and the state adjacency of one state map (phmrf_state_domains, phmrf_state_adjacency,
phylo_hmrf_amd.domains) against the full-matrix restatement of tests/domains_reference.py.  Everything is integer arithmetic:
every comparison is exact."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import domains_reference as D

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4
FILL = -7


@pytest.fixture(scope="module")
def gpu():
    import torch
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    return L, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _put(dev, x, dtype=np.uint8):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dtype))).to(dev)


def _adjacency(gpu, s, H, W, diag, K):
    from phylo_hmrf_amd import _lib
    L, dev, st = gpu
    s_t = _put(dev, s)
    out = np.full(K * K, FILL, dtype=np.int64)
    status = L.phmrf_state_adjacency(ctypes.c_void_p(s_t.data_ptr()), H, W, int(diag), K, _lib.ptr_i64(out), st)
    return status, out.reshape(K, K)


def _domains(gpu, s, H, W, diag, K, dist0=0, min_area=1, conf=None, capacity=None, want_out=True, want_comp=True,
             want_table=True, want_found=True):
    """-> (status, table rows written, n_domains, n_components, domain_out, the whole table buffer)"""
    from phylo_hmrf_amd import _lib
    L, dev, st = gpu
    n = len(s)
    s_t = _put(dev, s)
    c_t = None if conf is None else _put(dev, conf, np.float32)
    out_t = _put(dev, np.full(n, FILL), np.int32)
    capacity = n if capacity is None else capacity
    table = np.full((max(capacity, 1), 16), FILL, dtype=np.int64)
    comps = np.full(K, FILL, dtype=np.int64)
    found = ctypes.c_int64(FILL)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    status = L.phmrf_state_domains(ptr(s_t), ptr(c_t), H, W, int(diag), dist0, K, min_area, ptr(out_t) if want_out else None,
                                   capacity, _lib.ptr_i64(table) if want_table else None,
                                   ctypes.byref(found) if want_found else None, _lib.ptr_i64(comps) if want_comp else None, st)
    k = max(0, min(int(found.value), capacity))
    return status, table[:k], int(found.value), comps, out_t.cpu().numpy(), table


# ---- maps -----------------------------------------------------------------------------------------------------------------
def _nodes(M, diag):
    M = np.asarray(M)
    return M[np.triu_indices(M.shape[0])] if diag else M.reshape(-1)


def _blocky(rng, H, W, K):
    """a piecewise-constant map: constant tiles of 1 - 9 rows by 1 - 9 columns"""
    rows = np.repeat(np.arange(H), rng.integers(1, 10, H))[:H]
    cols = np.repeat(np.arange(W), rng.integers(1, 10, W))[:W]
    return rng.integers(0, K, (H, W))[rows][:, cols]


@functools.lru_cache(maxsize=None)
def _spiral(H, W):
    """a spiral one pixel wide from the corner inwards (state 1), one pixel between its arms (state 0)"""
    M = np.zeros((H, W), dtype=np.int64)
    i = j = 0
    di, dj = 0, 1
    M[0, 0] = 1

    def free(i, j, di, dj):
        a, b = i + di, j + dj
        if not (0 <= a < H and 0 <= b < W) or M[a, b]:
            return False
        a, b = a + di, b + dj
        return not (0 <= a < H and 0 <= b < W and M[a, b])

    while True:
        if not free(i, j, di, dj):
            di, dj = dj, -di
            if not free(i, j, di, dj):
                return M
        i, j = i + di, j + dj
        M[i, j] = 1


def _maps(H, W, diag, K, seed):
    """(name, node-order map) of one block: random, rectangles, one state, checkerboard, stripes along the diagonal, a
    spiral, and one state on 95 % of the nodes -- the kinds that need two states only where K allows them"""
    rng = np.random.default_rng(seed)
    ii, jj = np.indices((H, W))
    yield "random", _nodes(rng.integers(0, K, (H, W)), diag)
    yield "rectangles", _nodes(_blocky(rng, H, W, K), diag)
    yield "single", _nodes(np.full((H, W), K - 1), diag)
    if K >= 2:
        yield "checkerboard", _nodes((ii + jj) % 2 * (K - 1), diag)
        for t in (0, 1, 2):                                  # one stripe at j - i = t: the mirror rule's edge
            yield "stripe%d" % t, _nodes((jj - ii == t) * 1, diag)
        yield "stripes", _nodes(np.abs(jj - ii) // 2 % K, diag)
        yield "spiral", _nodes(_spiral(H, W) * (K - 1), diag)
        yield "dominant", _nodes(np.where(rng.random((H, W)) < 0.95, 0, rng.integers(1, K, (H, W))), diag)


def _conf(rng, n):
    c = rng.random(n).astype(np.float32)
    c[::7], c[::11], c[::13] = 0.5, 0.0, 1.0
    return c


def _listed(ref, min_area):
    """the reference's answer at min_area, from its answer at min_area 1"""
    keep = ref["table"][:, 6] >= min_area
    ident = np.where(keep, np.cumsum(keep) - 1, -1)
    return ref["table"][keep], ident[ref["domain_out"]].astype(np.int32)


def _check(gpu, s, H, W, diag, K, dist0=0, conf=None, what=""):
    """both entry points at min_area 1, 2 and above every area; -> the reference at min_area 1"""
    status, adj = _adjacency(gpu, s, H, W, diag, K)
    assert status == 0 and np.array_equal(adj, D.adjacency(s, H, W, diag, K)), what
    ref = D.region(s, H, W, diag, K, dist0, 1, conf)
    for min_area in (1, 2, int(ref["table"][:, 6].max()) + 1):
        status, table, found, comps, out, _ = _domains(gpu, s, H, W, diag, K, dist0, min_area, conf,
                                                       capacity=ref["table"].shape[0] + 1)
        want_table, want_out = _listed(ref, min_area)
        assert status == 0, what
        assert found == want_table.shape[0], (what, min_area, found, want_table.shape[0])
        assert np.array_equal(table, want_table), (what, min_area, np.argwhere(table != want_table)[:5].tolist())
        assert np.array_equal(out, want_out), (what, min_area)
        assert np.array_equal(comps, ref["n_components"]), (what, min_area)
    assert ref["table"][:, 8].sum() == 2 * np.triu(adj, 1).sum()
    return ref


def _block(gpu, H, W, diag, seed):
    for t, K in enumerate((1, 2, 20, 64)):
        for m, (name, s) in enumerate(_maps(H, W, diag, K, seed + K)):
            rng = np.random.default_rng(seed + 100 * m + K)
            conf = _conf(rng, s.size) if (t + m) % 2 == 0 else None
            dist0 = 0 if diag or m % 3 == 0 else int(rng.integers(-2 * H, 2 * W))
            _check(gpu, s, H, W, diag, K, dist0, conf, what=(name, H, W, diag, K, dist0, conf is not None))


@pytest.mark.parametrize("H", [1, 2, 3, 5, 8, 17, 64, 65, 130])
def test_diagonal_blocks(gpu, H):
    _block(gpu, H, H, True, H)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (5, 3), (64, 65), (130, 67)])
def test_off_diagonal_blocks(gpu, H, W):
    _block(gpu, H, W, False, 1000 * H + W)


def test_diagonal_block_with_a_distance_offset_and_confidences(gpu):
    """a diagonal block's own dist0 is 0; the call takes any, and |dist0 + j - i| folds where the sum changes sign"""
    rng = np.random.default_rng(5)
    s = _nodes(_blocky(rng, 40, 40, 5), True)
    for dist0 in (0, 9, -9, -100, 2 ** 31 - 50):
        _check(gpu, s, 40, 40, True, 5, dist0, _conf(rng, s.size), what=dist0)


# ---- the second trip of a wave: blocks past the capped grid -------------------------------------------------------------------
def test_sizes_lie_just_past_the_capped_grid():
    from phylo_hmrf_amd import domains
    cap = domains.GRID_CAP * 256                             # (GRID_CAP is pinned on the source, CPU test)
    assert cap < 513 * 513 < cap + 2048 and cap < 725 * 726 // 2 < cap + 2048
    assert 4096 * 256 < 1025 * 1025 < 4096 * 256 + 4096 and 4096 * 256 < 1450 * 1451 // 2     # launch_grid_components' grid


@pytest.mark.parametrize("H,W,diag", [(513, 513, False), (725, 725, True)])
@pytest.mark.parametrize("kind", ["dominant", "spiral", "rectangles"])
def test_just_past_the_capped_grid(gpu, H, W, diag, kind):
    """a wave owns more than 64 nodes: it carries a root from trip to trip, drops it and takes another"""
    s = dict((name, m) for name, m in _maps(H, W, diag, 20, 3))[kind]
    rng = np.random.default_rng(9)
    ref = _check(gpu, s, H, W, diag, 20, 0 if diag else -77, _conf(rng, s.size), what=kind)
    if kind == "dominant":
        assert ref["table"][:, 5].max() > 0.9 * s.size      # one root takes nearly every node


@pytest.mark.parametrize("H,W,diag", [(1025, 1025, False), (1450, 1450, True)])
def test_a_million_nodes(gpu, H, W, diag):
    rng = np.random.default_rng(H)
    M = _blocky(rng, H, W, 20)
    M[rng.random((H, W)) < 0.5] = 0                          # half of the map in one state, in one component
    s = _nodes(M, diag)
    ref = D.region(s, H, W, diag, 20, 31, 1, None)
    status, table, found, comps, out, _ = _domains(gpu, s, H, W, diag, 20, 31, 1, None, capacity=ref["table"].shape[0] + 1)
    assert status == 0 and found == ref["table"].shape[0]
    assert np.array_equal(table, ref["table"]) and np.array_equal(out, ref["domain_out"])
    assert np.array_equal(comps, ref["n_components"])
    status, adj = _adjacency(gpu, s, H, W, diag, 20)
    assert status == 0 and np.array_equal(adj, D.adjacency(s, H, W, diag, 20))


# ---- capacity, errors, determinism ------------------------------------------------------------------------------------------
def test_capacity_zero_and_a_capacity_below_the_count(gpu):
    rng = np.random.default_rng(11)
    s = _nodes(_blocky(rng, 65, 65, 20), True)
    conf = _conf(rng, s.size)
    ref = D.region(s, 65, 65, True, 20, 0, 1, conf)
    full, n_dom = ref["table"], ref["table"].shape[0]
    assert n_dom > 8
    for want_table in (True, False):                        # capacity 0 needs no table
        status, rows, found, comps, out, buf = _domains(gpu, s, 65, 65, True, 20, conf=conf, capacity=0, want_table=want_table)
        assert status == 0 and found == n_dom and (buf == FILL).all()
        assert np.array_equal(out, ref["domain_out"]) and np.array_equal(comps, ref["n_components"])
    for cap in (1, 5, n_dom - 1, n_dom, n_dom + 3):
        status, rows, found, comps, out, buf = _domains(gpu, s, 65, 65, True, 20, conf=conf, capacity=cap)
        assert status == 0 and found == n_dom
        assert np.array_equal(rows, full[:cap]) and (buf[min(cap, n_dom):] == FILL).all()
        assert np.array_equal(out, ref["domain_out"])       # the ids are given past the capacity too
    status, rows, found, comps, out, _ = _domains(gpu, s, 65, 65, True, 20, conf=conf, want_out=False, want_comp=False)
    assert status == 0 and np.array_equal(rows, full) and (out == FILL).all() and (comps == FILL).all()


def test_error_codes_leave_every_output_alone(gpu):
    rng = np.random.default_rng(2)
    s = _nodes(_blocky(rng, 17, 17, 6), True)
    s[5] = 5
    conf = _conf(rng, s.size)

    def status(*args, **kw):
        st, _, found, comps, out, buf = _domains(gpu, *args, **kw)
        if st != 0:
            assert found == FILL and (comps == FILL).all() and (out == FILL).all() and (buf == FILL).all()
        return st

    assert status(s, 17, 17, True, 6, conf=conf) == 0
    assert status(s, 17, 17, True, 5) == INVALID                                  # a label >= K
    assert status(s[:17 * 16], 17, 16, True, 6) == INVALID                        # a diagonal block is square
    assert status(s, 17, 17, True, 6, capacity=-1) == INVALID
    assert status(s, 17, 17, True, 6, min_area=0) == INVALID
    assert status(s, 17, 17, True, 6, want_table=False) == INVALID                # capacity > 0 without a table
    assert status(s, 17, 17, True, 6, want_found=False) == INVALID
    assert status(s, 17, 17, True, 0) == INVALID
    assert status(s, 0, 17, False, 6) == INVALID
    for bad in (np.nan, np.inf, -np.inf, 1.0000001, -1e-30, 2.0):
        c = conf.copy()
        c[-1] = bad
        assert status(s, 17, 17, True, 6, conf=c) == INVALID, bad
    c = conf.copy()
    c[3] = -0.0
    assert status(s, 17, 17, True, 6, conf=c) == 0
    assert status(s, 17, 17, True, 6, dist0=2 ** 31 - 17) == INVALID              # a distance of 2^31
    assert status(s, 17, 17, True, 6, dist0=-2 ** 31) == INVALID
    assert status(s, 17, 17, True, 6, dist0=2 ** 31 - 18) == 0
    assert status(s, 17, 17, True, 65) == UNSUPPORTED
    assert status(s, 46341, 46341, False, 6) == UNSUPPORTED                       # 2^31 - 64 nodes or more: checked first
    assert status(s, 65536, 65536, True, 6) == UNSUPPORTED

    def adj_status(*args):
        st, out = _adjacency(gpu, *args)
        if st != 0:
            assert (out == FILL).all()
        return st

    assert adj_status(s, 17, 17, True, 6) == 0
    assert adj_status(s, 17, 17, True, 5) == INVALID
    assert adj_status(s, 17, 16, True, 6) == INVALID
    assert adj_status(s, 17, 17, True, 65) == UNSUPPORTED
    assert adj_status(s, 46341, 46341, False, 6) == UNSUPPORTED
    L, dev, st = gpu
    out = np.full(36, FILL, dtype=np.int64)
    from phylo_hmrf_amd import _lib
    assert L.phmrf_state_adjacency(None, 17, 17, 1, 6, _lib.ptr_i64(out), st) == INVALID
    assert L.phmrf_state_adjacency(ctypes.c_void_p(_put(dev, s).data_ptr()), 17, 17, 1, 6, None, st) == INVALID
    assert (out == FILL).all()


def test_two_calls_give_the_same_bytes(gpu):
    s = dict((name, m) for name, m in _maps(513, 513, False, 20, 3))["dominant"]
    conf = _conf(np.random.default_rng(1), s.size)
    one = _domains(gpu, s, 513, 513, False, 20, 5, 1, conf)
    two = _domains(gpu, s, 513, 513, False, 20, 5, 1, conf)
    assert one[0] == two[0] == 0 and one[2] == two[2] > 0
    for x, y in zip(one[1:], two[1:]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    a, b = _adjacency(gpu, s, 513, 513, False, 20), _adjacency(gpu, s, 513, 513, False, 20)
    assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes()


# ---- against code that is already tested ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,diag", [(65, 65, True), (64, 65, False)])
def test_state_one_of_a_two_state_map_against_the_differential_domains(gpu, H, W, diag):
    """phmrf_diff_domains(a, zeros) lists the components of state 1: root, box, nodes and area are the new call's"""
    from phylo_hmrf_amd import _lib
    L, dev, st = gpu
    s = _nodes(_blocky(np.random.default_rng(H + W), H, W, 2), diag)
    a_t, z_t = _put(dev, s), _put(dev, np.zeros_like(s))
    old = np.full((s.size, 12), FILL, dtype=np.int64)
    found = ctypes.c_int64(FILL)
    assert L.phmrf_diff_domains(ctypes.c_void_p(a_t.data_ptr()), ctypes.c_void_p(z_t.data_ptr()), None, None, None, H, W,
                                int(diag), 0, 2, 2, 0.0, 1, None, s.size, _lib.ptr_i64(old), ctypes.byref(found), None, st) == 0
    status, table, _, _, _, _ = _domains(gpu, s, H, W, diag, 2)
    ones = table[table[:, 7] == 1]
    assert status == 0 and found.value == ones.shape[0] > 3
    assert np.array_equal(ones[:, :7], old[:found.value, :7])


def _islands(H, W):
    """state-1 rectangles of 1 - 6 rows and columns, one per cell of an 8 x 8 lattice and two cells of state 0 apart, so every
    one is a component: about sixty of them.  The ones in the lattice's diagonal cells cross the diagonal (a diagonal block:
    their own mirrors), the others lie clear of it (mirror twins).  One is a single node, one has a hole of a single node of
    state 0."""
    rng = np.random.default_rng(H * W)
    M = np.zeros((H, W), dtype=np.int64)
    for a in range(0, H - 7, 8):
        for b in range(0, W - 7, 8):
            h, w = rng.integers(1, 7, 2)
            M[a + 1:a + 1 + h, b + 1:b + 1 + w] = 1
    M[1:7, 25:31] = 0
    M[3, 27] = 1                                            # a single node, off the diagonal
    M[9:14, 33:38] = 1
    M[11, 35] = 0                                           # a hole: a single-node component of state 0
    return M


@pytest.mark.parametrize("H,W,diag", [(65, 65, True), (64, 65, False)])
def test_smoothing_comparison_and_domains_list_the_same_components(gpu, H, W, diag):
    """The three calls take their areas and the ids of their listed roots from one piece of code (csrc/components.h):
    the areas and node counts of state 1's domains are those of the differential domains of the map against zeros, and the
    smoothing's count of small components at max_area = A is the number of domains of either state with area <= A."""
    from phylo_hmrf_amd import _lib
    L, dev, st = gpu
    s = _nodes(_islands(H, W), diag)
    s_t, z_t = _put(dev, s), _put(dev, np.zeros_like(s))
    status, table, found, _, _, _ = _domains(gpu, s, H, W, diag, 2)
    assert status == 0 and found == table.shape[0] > 30
    ones, area, nodes = table[table[:, 7] == 1], table[:, 6], table[:, 5]
    assert (nodes == 1).sum() >= 2 and set(table[nodes == 1, 7]) == {0, 1}                # the single nodes of either state
    if diag:
        assert (ones[:, 6] > ones[:, 5]).sum() >= 5 and (ones[:, 6] == ones[:, 5]).sum() >= 20   # own mirrors, mirror twins

    old = np.full((s.size, 12), FILL, dtype=np.int64)
    n_old = ctypes.c_int64(FILL)
    assert L.phmrf_diff_domains(ctypes.c_void_p(s_t.data_ptr()), ctypes.c_void_p(z_t.data_ptr()), None, None, None, H, W,
                                int(diag), 0, 2, 2, 0.0, 1, None, s.size, _lib.ptr_i64(old), ctypes.byref(n_old), None, st) == 0
    assert n_old.value == ones.shape[0]
    assert np.array_equal(old[:n_old.value, 5], ones[:, 5]) and np.array_equal(old[:n_old.value, 6], ones[:, 6])

    out_t = _put(dev, np.zeros_like(s))
    small = []
    for A in (0, 1, 2, 8, 20, 36, 50, int(area.max())):
        counts = np.full(3, FILL, dtype=np.int64)
        assert L.phmrf_smooth_labels(ctypes.c_void_p(s_t.data_ptr()), ctypes.c_void_p(out_t.data_ptr()), H, W, int(diag), 2, 5, A,
                                     1, _lib.ptr_i64(counts), st) == 0
        assert counts[0] == (area <= A).sum(), (A, counts[0], (area <= A).sum())
        small.append(int(counts[0]))
    assert small[0] == 0 and small[-1] == found and len(set(small)) >= 6


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _two_regions():
    rng = np.random.default_rng(21)
    a = _nodes(_blocky(rng, 120, 120, 5), True)
    b = _nodes(_blocky(rng, 30, 45, 5), False)
    lv = np.array([[a.size, 0, a.size, 120, 120, 10, 10, 0, 1, 2],
                   [b.size, a.size, a.size + b.size, 30, 45, 10, 400, 1, 0, 2]])
    sv = np.concatenate([a, b])
    return sv, lv, _conf(rng, sv.size)


def _same(got, ref):
    assert sorted(got) == sorted(ref)
    for key in ref:
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key], equal_nan=True), key


def test_state_domains_on_two_regions(gpu):
    from phylo_hmrf_amd import domains
    sv, lv, conf = _two_regions()
    for c in (conf, None):
        for min_area in (None, 1, 7):
            _same(domains.state_domains(sv, lv, conf=c, min_area=min_area), D.state_vec_domains(sv, lv, conf=c, min_area=min_area))
    ref = D.state_vec_domains(sv, lv, min_area=1)
    assert ref["domains"][0, 0] == 0 and ref["domains"][-1, 0] == 1 and (ref["domain_vec"] >= 0).all()


def test_state_domains_asks_again_when_the_first_table_is_too_small(gpu):
    from phylo_hmrf_amd import domains
    s = np.random.default_rng(4).integers(0, 20, 513 * 513)
    lv = np.array([[s.size, 0, s.size, 513, 513, 0, 600, 0, 0, 1]])
    got, ref = domains.state_domains(s, lv, min_area=1), D.state_vec_domains(s, lv, min_area=1)
    assert ref["domains"].shape[0] > domains.FIRST_CAPACITY
    _same(got, ref)


def test_command_line_writes_the_files_of_the_reference(gpu, tmp_path):
    import scipy.io
    import phylo_hmrf as cli
    sv, lv, conf = _two_regions()
    smooth = np.where(sv == 4, 0, sv)
    path = str(tmp_path / "segment_7_5.mat")
    scipy.io.savemat(path, dict(state_vec=sv.reshape(1, -1), state_vec_smooth=smooth.reshape(1, -1), len_vec=lv,
                                conf=conf.reshape(1, -1)))
    out = str(tmp_path / "out")

    def run(**extra):
        return cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                       "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", out, quiet="1",
                       domains=path, **extra)

    for states, extra, area in ((sv, dict(), None), (smooth, dict(domains_field="state_vec_smooth", domains_area="3"), 3)):
        written = run(**extra)
        assert written == os.path.join(out, "domains_segment_7_5.mat")
        ref = D.state_vec_domains(states, lv, conf=conf, min_area=area)
        mat = scipy.io.loadmat(written)
        for key in ref:
            assert np.array_equal(np.asarray(mat[key]).reshape(ref[key].shape), ref[key], equal_nan=True), key
        assert mat["domains_area"].reshape(-1).tolist() == ([81, 26] if area is None else [3, 3])
        assert int(mat["resolution"].reshape(-1)[0]) == 50000
        text = open(os.path.join(out, "domains_segment_7_5.txt"), "rb").read().decode()
        assert text == D.lines(ref["domains"], ref["domain_conf"], lv, 50000)
        assert text.count("\n") == ref["domains"].shape[0] + 1 > 3
