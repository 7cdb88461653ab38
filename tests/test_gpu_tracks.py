"""GPU: the genome tracks of one state map (phmrf_state_tracks, phylo_hmrf_amd.tracks) against the full-matrix restatement of
tests/tracks_reference.py.  Everything is integer arithmetic: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

from phylo_hmrf_amd import tracks
from tests import tracks_reference as R

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4
FILL = 0xA5
WINDOWS = ((0, -1), (0, 0), (1, 1), (3, 17))


@pytest.fixture(scope="module")
def gpu():
    import torch
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    return L, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _filled(count):
    return np.full(8 * count, FILL, dtype=np.uint8).view(np.int64)


def _untouched(a):
    return bool(np.all(a.view(np.uint8) == FILL))


def _call(gpu, labels, H, W, diag, dist0, K, d_min, d_max, offset=0, no_labels=False, no_rows=False, no_cols=False, small=False):
    """-> (status, rows int64 [H, K], cols int64 [W, K]); both buffers are filled with FILL before the call.  The labels start
    `offset` bytes into their device buffer.  small: a call that must be refused, with one-word buffers."""
    import torch
    L, dev, st = gpu
    h, w, k = max(H, 1), max(W, 1), max(K, 1)
    rows = _filled(1 if small else h * k)
    cols = _filled(1 if small else w * k)
    a = np.zeros(offset + len(labels), dtype=np.uint8)
    a[offset:] = labels
    s_t = torch.from_numpy(a).to(dev)[offset:]
    status = L.phmrf_state_tracks(None if no_labels else ctypes.c_void_p(s_t.data_ptr()), H, W, int(diag), dist0, K, d_min, d_max,
                                  None if no_rows else rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  None if no_cols else cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), st)
    if not small:
        rows, cols = rows.reshape(h, k), cols.reshape(w, k)
    return status, rows, cols


def _check(gpu, labels, H, W, diag, dist0, K, d_min, d_max, offset=0, what="", ref=None):
    status, rows, cols = _call(gpu, labels, H, W, diag, dist0, K, d_min, d_max, offset)
    what = (what, H, W, diag, dist0, K, d_min, d_max, offset)
    assert status == 0, what
    want = R.tracks(labels, H, W, diag, dist0, K, d_min, d_max) if ref is None else ref
    assert np.array_equal(rows, want[0]), (what, "rows", np.argwhere(rows != want[0])[:5].tolist())
    if diag:
        assert _untouched(cols), what                        # a diagonal block: only rows is written
    else:
        assert np.array_equal(cols, want[1]), (what, "cols", np.argwhere(cols != want[1])[:5].tolist())
    return rows, cols


# ---- maps -------------------------------------------------------------------------------------------------------------------
def _nodes(M, diag):
    M = np.asarray(M)
    return (M[np.triu_indices(M.shape[0])] if diag else M.reshape(-1)).astype(np.uint8)


def _blocky(rng, H, W, K):
    """a piecewise-constant map: constant tiles of 1 - 9 rows by 1 - 9 columns"""
    rows = np.repeat(np.arange(H), rng.integers(1, 10, H))[:H]
    cols = np.repeat(np.arange(W), rng.integers(1, 10, W))[:W]
    return rng.integers(0, K, (H, W))[rows][:, cols]


KINDS = ("random", "blocky", "constant", "rows", "columns")


def _map(kind, H, W, diag, K, seed):
    rng = np.random.default_rng(seed)
    ii, jj = np.indices((H, W))
    if kind == "random":
        M = rng.integers(0, K, (H, W))
    elif kind == "blocky":
        M = _blocky(rng, H, W, K)
    elif kind == "constant":
        M = np.full((H, W), K - 1)
    elif kind == "rows":                                     # single-row stripes: every storage row in a state of its own
        M = ii % K
    elif kind == "columns":                                  # single-column stripes
        M = jj % K
    else:
        raise ValueError(kind)
    return _nodes(M, diag)


def _beyond(H, W, dist0):
    return abs(dist0) + H + W + 5


# ---- shapes and forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, 2, 5, 63, 64, 65, 130, 257])
def test_diagonal_blocks(gpu, side):
    """sides around the tile's height (32), two of its heights (64) and its width (256), and the smallest blocks there are"""
    labels = _map("random", side, side, True, 20, side)
    for d_min, d_max in WINDOWS:
        rows, _ = _check(gpu, labels, side, side, True, 0, 20, d_min, d_max)
        if (d_min, d_max) == (0, -1):
            assert rows.sum() == side * side
    status, rows, _ = _call(gpu, labels, side, side, True, 0, 20, _beyond(side, side, 0), -1)
    assert status == 0 and not rows.any()


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (63, 65), (65, 130), (257, 300)])
def test_off_diagonal_blocks(gpu, H, W):
    labels = _map("random", H, W, False, 20, H * 1000 + W)
    for dist0 in (0, 5, -3, 1000, -(W + 10)):
        near = (max(0, abs(dist0) - 2), abs(dist0) + 20)     # a window that cuts through the block wherever dist0 puts it
        for d_min, d_max in WINDOWS + (near,):
            rows, cols = _check(gpu, labels, H, W, False, dist0, 20, d_min, d_max)
            if (d_min, d_max) == (0, -1):
                assert rows.sum() == H * W and cols.sum() == H * W
        status, rows, cols = _call(gpu, labels, H, W, False, dist0, 20, _beyond(H, W, dist0), -1)
        assert status == 0 and not rows.any() and not cols.any()


@pytest.mark.parametrize("K", [1, 2, 20, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_map_types_and_state_counts(gpu, kind, K):
    for H, W, diag, dist0 in ((130, 130, True, 0), (65, 130, False, 7)):
        labels = _map(kind, H, W, diag, K, K)
        for d_min, d_max in ((0, -1), (3, 17)):
            _check(gpu, labels, H, W, diag, dist0, K, d_min, d_max, what=kind)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_label_slices_start_at_any_byte(gpu, offset):
    """a region's slice of a state_vec: heads of 0 - 3 bytes before the first 4-byte word of every storage row"""
    for H, W, diag in ((65, 65, True), (63, 65, False), (5, 300, False), (9, 3, False)):
        for kind in ("random", "blocky"):
            labels = _map(kind, H, W, diag, 20, offset + H)
            _check(gpu, labels, H, W, diag, 0, 20, 0, -1, offset=offset, what=kind)
            _check(gpu, labels, H, W, diag, 0, 20, 2, 40, offset=offset, what=kind)


# ---- windows at the tile's bounds -------------------------------------------------------------------------------------------
def _tile_windows():
    out = []
    for bound in (tracks.TILE_H, tracks.TILE_W):
        for b in (bound - 1, bound, bound + 1):
            out += [(b, -1), (0, b), (b, b)]
    out.append((tracks.TILE_H, tracks.TILE_W))
    return out


@pytest.mark.parametrize("H,W,diag,dist0", [(2 * tracks.TILE_W + 8, 2 * tracks.TILE_W + 8, True, 0),
                                            (2 * tracks.TILE_H + 6, 2 * tracks.TILE_W + 88, False, 0),
                                            (2 * tracks.TILE_H + 6, tracks.TILE_W + 3, False, -tracks.TILE_H)])
def test_windows_at_the_tile_bounds(gpu, H, W, diag, dist0):
    """windows whose bounds sit at the tile's height and width and one either side: tiles wholly outside the window (not
    read), wholly inside it (no per-cell test) and cut by it lie side by side"""
    labels = _map("blocky", H, W, diag, 20, H + W)
    for d_min, d_max in _tile_windows():
        _check(gpu, labels, H, W, diag, dist0, 20, d_min, d_max)


# ---- the grid stride --------------------------------------------------------------------------------------------------------
def test_more_tiles_than_twice_the_grid_cap(gpu):
    H, W = tracks.TILE_H * (2 * tracks.GRID_CAP + 1) + 5, 3             # 2 cap + 2 tiles of one tile column
    assert -(-H // tracks.TILE_H) * -(-W // tracks.TILE_W) > 2 * tracks.GRID_CAP
    labels = _map("blocky", H, W, False, 20, 3)
    _check(gpu, labels, H, W, False, 5, 20, 0, -1)
    _check(gpu, labels, H, W, False, 5, 20, 40000, 50000)


@pytest.fixture(scope="module")
def large():
    side = 2300                                              # 2.6 M nodes
    return side, _map("blocky", side, side, True, 20, 23)


@pytest.mark.parametrize("window", [(0, -1), (0, 200), (300, 1500)])
def test_large_diagonal_block(gpu, large, window):
    side, labels = large
    rows, _ = _check(gpu, labels, side, side, True, 0, 20, window[0], window[1])
    if window == (0, -1):
        assert rows.sum() == side * side == 2 * labels.size - side


# ---- bad labels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,diag,dist0", [(70, 70, True, 0), (40, 300, False, 3)])
def test_bad_label_inside_and_outside_the_window(gpu, H, W, diag, dist0):
    good = _map("random", H, W, diag, 5, 9)
    i, j = 2, 33                                             # distance |dist0 + 31|
    d = abs(dist0 + j - i)
    at = i * W - i * (i - 1) // 2 + (j - i) if diag else i * W + j
    for bad_state in (5, 64, 255):
        labels = good.copy()
        labels[at] = bad_state
        for d_min, d_max in ((0, -1), (d, d), (0, d), (d, -1)):
            status, rows, cols = _call(gpu, labels, H, W, diag, dist0, 5, d_min, d_max)
            assert status == INVALID and _untouched(rows) and _untouched(cols), (bad_state, d_min, d_max)
        for d_min, d_max in ((0, d - 1), (d + 1, -1), (d + 1, d + 1)):
            # (the restatement on the good map: the bad cell lies outside the window and counts for nothing)
            _check(gpu, labels, H, W, diag, dist0, 5, d_min, d_max, ref=R.tracks(good, H, W, diag, dist0, 5, d_min, d_max))


# ---- argument refusals ------------------------------------------------------------------------------------------------------
def test_refused_arguments_write_nothing(gpu):
    lab = np.zeros(64, dtype=np.uint8)
    ok = dict(labels=lab, H=4, W=5, diag=False, dist0=0, K=3, d_min=0, d_max=-1)
    assert _call(gpu, **ok)[0] == 0
    cases = [
        (dict(no_labels=True), INVALID),
        (dict(no_rows=True), INVALID),
        (dict(no_cols=True), INVALID),                       # an off-diagonal block needs cols
        (dict(H=0), INVALID), (dict(W=0), INVALID), (dict(H=-2), INVALID), (dict(K=0), INVALID), (dict(K=-1), INVALID),
        (dict(diag=True), INVALID),                          # 4 x 5: not square
        (dict(diag=True, W=4, dist0=1), INVALID),            # a diagonal block with dist0 != 0
        (dict(diag=True, W=4, dist0=-1), INVALID),
        (dict(d_min=-1), INVALID),
        (dict(d_min=3, d_max=2), INVALID),
        (dict(d_min=0, d_max=-2), INVALID),
        (dict(K=65), UNSUPPORTED),
        (dict(diag=True, H=65536, W=65536, small=True), UNSUPPORTED),           # n = 2^31 + 2^15
        (dict(H=46341, W=46341, small=True), UNSUPPORTED),                      # n = 2,147,488,281
        (dict(dist0=(1 << 31) - 9), UNSUPPORTED),                               # |dist0| + H + W = 2^31
        (dict(dist0=-((1 << 31) - 9)), UNSUPPORTED),
        (dict(dist0=1 << 40), UNSUPPORTED),
    ]
    for change, want in cases:
        status, rows, cols = _call(gpu, **dict(ok, **change))
        assert status == want, change
        assert _untouched(rows) and _untouched(cols), change
    # the largest distances that are supported, and a diagonal block without cols
    assert _call(gpu, **dict(ok, dist0=(1 << 31) - 10))[0] == 0
    status, rows, _ = _call(gpu, **dict(ok, diag=True, W=4, no_cols=True))
    assert status == 0 and rows.sum() == 16


def test_huge_window_bounds_are_no_error(gpu):
    labels = _map("random", 40, 50, False, 4, 1)
    _check(gpu, labels, 40, 50, False, 2, 4, 0, 1 << 40)                        # as good as no upper limit
    _check(gpu, labels, 40, 50, False, 2, 4, 1 << 40, -1)                       # nothing inside
    _check(gpu, labels, 40, 50, False, 2, 4, 1 << 40, 1 << 41)


# ---- other properties -------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes(gpu):
    for H, W, diag in ((300, 300, True), (100, 600, False)):
        labels = _map("random", H, W, diag, 20, 4)
        a = _call(gpu, labels, H, W, diag, 0, 20, 1, 280)
        b = _call(gpu, labels, H, W, diag, 0, 20, 1, 280)
        assert a[0] == 0 and b[0] == 0
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_row_totals_are_the_contingency_diagonal(gpu):
    from phylo_hmrf_amd import compare
    H, W, K = 90, 310, 11
    labels = _map("blocky", H, W, False, K, 8)
    status, rows, cols = _call(gpu, labels, H, W, False, 12, K, 0, -1)
    assert status == 0
    C = compare.contingency(labels, labels, K, K)
    assert np.array_equal(rows.sum(axis=0), np.diagonal(C)) and np.array_equal(cols.sum(axis=0), np.diagonal(C))


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _genome():
    """chromosome 1: diagonal regions at bins 0 and 90 and the off-diagonal region between them; chromosome 2: one diagonal
    region that starts at bin 4"""
    shapes = [(70, 70, 1, 0, 0, 1), (70, 45, 0, 0, 90, 1), (45, 45, 1, 90, 90, 1), (33, 33, 1, 4, 4, 2)]
    parts, rows, at = [], [], 0
    for r, (H, W, diag, s1, s2, chrom) in enumerate(shapes):
        lab = _map("blocky", H, W, bool(diag), 6, r)
        parts.append(lab)
        rows.append([lab.size, at, at + lab.size, H, W, s1, s2, r, diag, chrom])
        at += lab.size
    return np.concatenate(parts), np.array(rows, dtype=np.int64)


def test_state_tracks_end_to_end():
    s, L = _genome()
    windows = [(0, -1), (2, 60)]
    got = tracks.state_tracks(s, L, windows=windows)
    ref = R.state_tracks(s, L, windows, 6)
    assert got["chrom"].tolist() == [1, 2] and got["windows"].tolist() == [[0, -1], [2, 60]]
    assert sorted(got) == sorted(list(ref) + ["windows"])
    for name in ref:
        assert got[name].dtype == np.int64 and np.array_equal(got[name], ref[name]), name
    assert got["track_1"].shape == (2, 135, 6) and got["track_2"].shape == (2, 37, 6)
    assert not got["track_1"][:, 70:90].any() and not got["track_2"][:, :4].any()
    wide = tracks.state_tracks(s.reshape(1, -1).astype(np.float64), L, K=9)    # as a .mat file holds them
    assert wide["track_1"].shape == (1, 135, 9) and np.array_equal(wide["track_1"][0, :, :6], ref["track_1"][0])
    with pytest.raises(RuntimeError):
        tracks.state_tracks(s, L, K=3)                       # a state >= K inside the window
    with pytest.raises(ValueError):
        tracks.state_tracks(s, L, windows=[(4, 2)])


def test_tracks_files_round_trip(tmp_path):
    import scipy.io
    s, L = _genome()
    path = os.path.join(str(tmp_path), "estimate_ou_7.mat")
    scipy.io.savemat(path, dict(state_vec=s.reshape(1, -1), state_vec_smooth=(5 - s).reshape(1, -1), len_vec=L))
    out = tracks.tracks_files(path, str(tmp_path / "out"), 50000, field="state_vec_smooth", windows_bp="0-,100000-3000000")
    assert os.path.basename(out) == "tracks_estimate_ou_7.npz"
    z = np.load(out, allow_pickle=False)
    ref = R.state_tracks(5 - s, L, [(0, -1), (2, 60)], 6)
    for name in ref:
        assert np.array_equal(z[name], ref[name]), name
    assert z["windows"].tolist() == [[0, -1], [2, 60]] and np.array_equal(z["len_vec"], L)
    assert int(z["resolution"]) == 50000 and str(z["tracks_field"]) == "state_vec_smooth"
    for q in (0, 1):
        lines = open(os.path.join(str(tmp_path / "out"), "tracks_estimate_ou_7_w%d.txt" % q)).read().splitlines()
        assert lines[0].startswith("#chrom\tstart\tstop\ttotal\tdominant\tshare\tentropy\tswitch\tstate1") and lines[0].endswith("state6")
        cells = [ln.split("\t") for ln in lines[1:]]
        assert len(cells) == 70 + 45 + 33                    # the covered bins
        keys = [(int(c[0]), int(c[1])) for c in cells]
        assert keys == sorted(keys) and all(int(c[2]) == int(c[1]) + 50000 for c in cells)
        for c in cells:
            counts = ref["track_%s" % c[0]][q][int(c[1]) // 50000]
            assert [int(x) for x in c[8:]] == counts.tolist() and int(c[3]) == counts.sum()
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["tracks_estimate_ou_7.npz", "tracks_estimate_ou_7_w0.txt",
                                                         "tracks_estimate_ou_7_w1.txt"]
