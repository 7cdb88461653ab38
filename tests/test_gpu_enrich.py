"""GPU: the pair enrichment of one state map (phmrf_pair_enrichment, phylo_hmrf_amd.enrich) against the restatement over the
full index arrays of tests/enrich_reference.py.  Everything is integer arithmetic: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

from phylo_hmrf_amd import enrich
from tests import enrich_reference as R

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


def _untouched(*tables):
    return all(bool(np.all(a.view(np.uint8) == FILL)) for a in tables)


def _call(gpu, labels, H, W, diag, dist0, K, C, row_class, col_class=None, row_seg=None, col_seg=None, d_min=0, d_max=-1, d_lo=0,
          D=0, offset=0, null=(), small=False):
    """-> (status, obs int64 [2 C C, K], state_dist int64 [D, K], cat_dist int64 [D, 2 C C]); the three buffers are filled with
    FILL before the call.  The labels start `offset` bytes into their device buffer.  null: names of pointers passed as NULL.
    small: a call that must be refused, with one-word buffers."""
    import torch
    L, dev, st = gpu
    k, c, d = max(K, 1), max(C, 1), max(D, 0)
    P = 2 * c * c
    obs, sd, cd = (_filled(1 if small else max(1, x)) for x in (P * k, d * k, d * P))
    a = np.zeros(offset + len(labels), dtype=np.uint8)
    a[offset:] = labels
    held = [torch.from_numpy(a).to(dev)[offset:]]

    def up(name, x, dtype):
        if x is None or name in null:
            return None
        held.append(torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(dev))
        return ctypes.c_void_p(held[-1].data_ptr())

    out = lambda name, x: None if name in null else x.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    status = L.phmrf_pair_enrichment(None if "labels" in null else ctypes.c_void_p(held[0].data_ptr()), H, W, int(diag), dist0, K, C,
                                     up("row_class", row_class, np.uint8), up("col_class", col_class, np.uint8),
                                     up("row_seg", row_seg, np.int32), up("col_seg", col_seg, np.int32), d_min, d_max, d_lo, D,
                                     out("obs", obs), out("state_dist", sd), out("cat_dist", cd), st)
    if not small and status == 0:
        obs, sd, cd = obs[:P * k].reshape(P, k), sd[:d * k].reshape(d, k), cd[:d * P].reshape(d, P)
    return status, obs, sd, cd


def _check(gpu, labels, H, W, diag, dist0, K, C, row_class, col_class=None, row_seg=None, col_seg=None, d_min=0, d_max=-1, offset=0,
           what="", ref=None, slack=0):
    """the call on the tight table range (widened by `slack` distances at both ends) against the restatement, and the
    identities that hold between the three tables"""
    rng = enrich.distance_range(H, W, diag, dist0, d_min, d_max)
    d_lo, D = (d_min, 0) if rng is None else rng
    d_lo, D = max(0, d_lo - slack), D + slack + (d_lo - max(0, d_lo - slack))
    status, obs, sd, cd = _call(gpu, labels, H, W, diag, dist0, K, C, row_class, col_class, row_seg, col_seg, d_min, d_max, d_lo, D,
                                offset)
    what = (what, H, W, diag, dist0, K, C, d_min, d_max, offset)
    assert status == 0, what
    want = R.tables(labels, H, W, diag, dist0, K, C, row_class, col_class, row_seg, col_seg, d_min, d_max, d_lo, D) if ref is None else ref
    for name, got, ref_table in zip(("obs", "state_dist", "cat_dist"), (obs, sd, cd), want):
        assert got.shape == ref_table.shape and np.array_equal(got, ref_table), (what, name, np.argwhere(got != ref_table)[:5].tolist())
    assert obs.sum() == sd.sum() == cd.sum()
    assert np.array_equal(obs.sum(axis=1), cd.sum(axis=0)) and np.array_equal(obs.sum(axis=0), sd.sum(axis=0))
    return obs, sd, cd


# ---- maps and annotations ---------------------------------------------------------------------------------------------------
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


def _intervals(rng, n, lo, hi):
    """values in [lo, hi) constant over intervals of 3 - 20 bins"""
    lengths = rng.integers(3, 21, n // 3 + 1)
    return np.repeat(rng.integers(lo, hi, lengths.shape[0]), lengths)[:n]


ANNOTATIONS = ("per_bin", "intervals", "none", "one")
SEGMENTS = ("absent", "given", "all_none")


def _classes(kind, n, C, seed):
    rng = np.random.default_rng(seed)
    if kind == "per_bin":                                    # runs of length 1
        return rng.integers(0, C, n).astype(np.uint8)
    if kind == "intervals":
        return _intervals(rng, n, 0, C).astype(np.uint8)
    return np.full(n, 0 if kind == "none" else C - 1, dtype=np.uint8)


def _segs(kind, n, seed):
    """few ids, so that row and column bins of an off-diagonal block meet in one segment"""
    if kind == "absent":
        return None
    return _intervals(np.random.default_rng(seed), n, -1, 6).astype(np.int32) if kind == "given" else np.full(n, -1, dtype=np.int32)


def _annotation(H, W, diag, C, seed, classes="intervals", segments="given"):
    """-> dict(row_class, col_class, row_seg, col_seg); a diagonal block has no column arrays"""
    out = dict(row_class=_classes(classes, H, C, seed), row_seg=_segs(segments, H, seed + 1), col_class=None, col_seg=None)
    if not diag:
        out.update(col_class=_classes(classes, W, C, seed + 2), col_seg=_segs(segments, W, seed + 3))
    return out


def _beyond(H, W, dist0):
    return abs(dist0) + H + W + 5


# ---- shapes and forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, 2, 5, 31, 32, 33, 63, 65, 127, 128, 129, 257])
def test_diagonal_blocks(gpu, side):
    """sides around the tile's height (32), two of its heights, its width (128) and two of its widths, and the smallest"""
    labels = _map("random", side, side, True, 20, side)
    ann = _annotation(side, side, True, 3, side)
    for d_min, d_max in WINDOWS:
        obs, _, _ = _check(gpu, labels, side, side, True, 0, 20, 3, d_min=d_min, d_max=d_max, **ann)
        if (d_min, d_max) == (0, -1):
            assert obs.sum() == side * (side + 1) // 2       # stored nodes count once
    status, obs, sd, cd = _call(gpu, labels, side, side, True, 0, 20, 3, d_min=_beyond(side, side, 0), D=4, **ann)
    assert status == 0 and not obs.any() and not sd.any() and not cd.any() and sd.shape == (4, 20)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (63, 65), (65, 130), (257, 300)])
def test_off_diagonal_blocks(gpu, H, W):
    """dist0 -3 and -(W // 2): two signed diagonals of one tile fold onto one distance"""
    labels = _map("random", H, W, False, 20, H * 1000 + W)
    ann = _annotation(H, W, False, 3, H + W)
    for dist0 in (0, 5, -3, 1000, -(W + 10), -(W // 2)):
        near = (max(0, abs(dist0) - 2), abs(dist0) + 20)     # a window that cuts through the block wherever dist0 puts it
        for d_min, d_max in WINDOWS + (near,):
            obs, _, _ = _check(gpu, labels, H, W, False, dist0, 20, 3, d_min=d_min, d_max=d_max, **ann)
            if (d_min, d_max) == (0, -1):
                assert obs.sum() == H * W
        status, obs, sd, cd = _call(gpu, labels, H, W, False, dist0, 20, 3, d_min=_beyond(H, W, dist0), **ann)
        assert status == 0 and not obs.any() and sd.size == 0 and cd.size == 0


@pytest.mark.parametrize("C", [1, 2, 8])
@pytest.mark.parametrize("K", [1, 2, 20, 64])
def test_state_and_class_counts_with_every_map_and_annotation(gpu, K, C):
    """(K = 64, C = 8 on the 130-bin block is the largest LDS configuration)"""
    for H, W, diag, dist0 in ((130, 130, True, 0), (65, 130, False, -7)):
        for m, kind in enumerate(KINDS):
            labels = _map(kind, H, W, diag, K, K + m)
            for a, classes in enumerate(ANNOTATIONS):
                segments = SEGMENTS[(m + a) % 3]
                ann = _annotation(H, W, diag, C, 10 * m + a, classes, segments)
                for d_min, d_max in ((0, -1), (3, 17)):
                    _check(gpu, labels, H, W, diag, dist0, K, C, d_min=d_min, d_max=d_max, what=(kind, classes, segments), **ann)


@pytest.mark.parametrize("segments", SEGMENTS)
def test_segments_with_every_annotation(gpu, segments):
    for H, W, diag, dist0 in ((130, 130, True, 0), (65, 130, False, 20)):
        labels = _map("blocky", H, W, diag, 20, 5)
        for a, classes in enumerate(ANNOTATIONS):
            ann = _annotation(H, W, diag, 4, a, classes, segments)
            obs, _, _ = _check(gpu, labels, H, W, diag, dist0, 20, 4, what=(classes, segments), **ann)
            inside = obs.reshape(4, 4, 2, 20)[:, :, 1].sum()
            assert (inside > 0) == (segments == "given")


def test_largest_lds_configuration_fills_every_category(gpu):
    side, K, C = 130, 64, 8
    labels = _map("random", side, side, True, K, 1)
    ann = _annotation(side, side, True, C, 2, "per_bin", "given")
    obs, _, _ = _check(gpu, labels, side, side, True, 0, K, C, **ann)
    assert (obs.reshape(C, C, 2, K)[:, :, 0].sum(axis=2) > 0).all() and obs.sum() == side * (side + 1) // 2


def test_a_diagonal_block_ignores_the_column_pointers(gpu):
    labels = _map("blocky", 70, 70, True, 6, 3)
    ann = _annotation(70, 70, True, 3, 4)
    want = R.tables(labels, 70, 70, True, 0, 6, 3, ann["row_class"], None, ann["row_seg"], None)
    junk = dict(ann, col_class=np.full(70, 200, dtype=np.uint8), col_seg=np.full(70, 1, dtype=np.int32))
    _check(gpu, labels, 70, 70, True, 0, 6, 3, ref=want, **junk)
    _check(gpu, labels, 70, 70, True, 0, 6, 3, ref=want, **dict(ann, col_seg=np.full(70, 1, dtype=np.int32)))


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_label_slices_start_at_any_byte(gpu, offset):
    """a region's slice of a state_vec: heads of 0 - 3 bytes before the first 4-byte word of every storage row"""
    for H, W, diag in ((65, 65, True), (63, 65, False), (5, 300, False), (9, 3, False)):
        ann = _annotation(H, W, diag, 3, H)
        for kind in ("random", "blocky"):
            labels = _map(kind, H, W, diag, 20, offset + H)
            _check(gpu, labels, H, W, diag, 0, 20, 3, offset=offset, what=kind, **ann)
            _check(gpu, labels, H, W, diag, 0, 20, 3, d_min=2, d_max=40, offset=offset, what=kind, **ann)


def test_a_wider_table_than_the_window_needs(gpu):
    labels = _map("blocky", 90, 140, False, 7, 2)
    ann = _annotation(90, 140, False, 3, 6)
    for dist0, d_min, d_max in ((0, 0, -1), (-40, 5, 60), (300, 0, 320)):
        _check(gpu, labels, 90, 140, False, dist0, 7, 3, d_min=d_min, d_max=d_max, slack=9, **ann)


# ---- windows at the tile's bounds -------------------------------------------------------------------------------------------
def _tile_windows():
    out = []
    for bound in (enrich.TILE_H, enrich.TILE_W):
        for b in (bound - 1, bound, bound + 1):
            out += [(b, -1), (0, b), (b, b)]
    out.append((enrich.TILE_H, enrich.TILE_W))
    return out


@pytest.mark.parametrize("H,W,diag,dist0", [(2 * enrich.TILE_W + 8, 2 * enrich.TILE_W + 8, True, 0),
                                            (2 * enrich.TILE_H + 6, 2 * enrich.TILE_W + 88, False, 0),
                                            (2 * enrich.TILE_H + 6, enrich.TILE_W + 3, False, -enrich.TILE_H)])
def test_windows_at_the_tile_bounds(gpu, H, W, diag, dist0):
    """tiles wholly outside the window (not read), wholly inside it (no per-cell test) and cut by it lie side by side"""
    labels = _map("blocky", H, W, diag, 20, H + W)
    ann = _annotation(H, W, diag, 3, H)
    for d_min, d_max in _tile_windows():
        _check(gpu, labels, H, W, diag, dist0, 20, 3, d_min=d_min, d_max=d_max, **ann)


# ---- the grid stride --------------------------------------------------------------------------------------------------------
def test_more_tiles_than_the_grid_cap(gpu):
    """the stride's second trip runs in both kernels"""
    H = W = 2200
    assert -(-H // enrich.TILE_H) * -(-W // enrich.TILE_W) > enrich.GRID_CAP
    assert (H + W - 1) * -(-H // enrich.CHUNK) > 4 * enrich.GRID_CAP
    labels = _map("blocky", H, W, False, 20, 3)
    ann = _annotation(H, W, False, 3, 8)
    obs, _, _ = _check(gpu, labels, H, W, False, -40, 20, 3, **ann)
    assert obs.sum() == H * W


@pytest.fixture(scope="module")
def large():
    side = 1500                                              # 1.1 M nodes
    return side, _map("blocky", side, side, True, 20, 23), _annotation(side, side, True, 3, 24)


@pytest.mark.parametrize("window", [(0, -1), (0, 200), (300, 900)])
def test_large_diagonal_block(gpu, large, window):
    side, labels, ann = large
    _check(gpu, labels, side, side, True, 0, 20, 3, d_min=window[0], d_max=window[1], **ann)


# ---- bad labels and classes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,diag,dist0", [(70, 70, True, 0), (40, 300, False, 3)])
def test_bad_label_inside_and_outside_the_window(gpu, H, W, diag, dist0):
    good = _map("random", H, W, diag, 5, 9)
    ann = _annotation(H, W, diag, 3, 1)
    i, j = 2, 33                                             # distance |dist0 + 31|
    d = abs(dist0 + j - i)
    at = i * W - i * (i - 1) // 2 + (j - i) if diag else i * W + j
    for bad_state in (5, 64, 255):
        labels = good.copy()
        labels[at] = bad_state
        for d_min, d_max in ((0, -1), (d, d), (0, d), (d, -1)):
            d_lo, D = enrich.distance_range(H, W, diag, dist0, d_min, d_max)
            status, obs, sd, cd = _call(gpu, labels, H, W, diag, dist0, 5, 3, d_min=d_min, d_max=d_max, d_lo=d_lo, D=D, **ann)
            assert status == INVALID and _untouched(obs, sd, cd), (bad_state, d_min, d_max)
        for d_min, d_max in ((0, d - 1), (d + 1, -1), (d + 1, d + 1)):
            # (the restatement on the good map: the bad node lies outside the window and counts for nothing)
            rng = enrich.distance_range(H, W, diag, dist0, d_min, d_max)
            want = R.tables(good, H, W, diag, dist0, 5, 3, d_min=d_min, d_max=d_max, d_lo=rng[0], D=rng[1], **ann)
            _check(gpu, labels, H, W, diag, dist0, 5, 3, d_min=d_min, d_max=d_max, ref=want, **ann)


def test_bad_class_inside_and_outside_the_window(gpu):
    H, W, dist0, C = 40, 300, 1000, 3
    labels = _map("blocky", H, W, False, 5, 2)
    good = _annotation(H, W, False, C, 3)
    cut = dist0 + W - 1 - 2                                  # d >= cut: the nodes with j - i >= W - 3, so rows 0 - 2 and columns W - 3 ...
    for where, index, inside in (("row_class", 1, True), ("row_class", 10, False), ("col_class", W - 2, True),
                                 ("col_class", 100, False)):
        for value in (C, 255):
            ann = dict(good, **{where: good[where].copy()})
            ann[where][index] = value
            status, obs, sd, cd = _call(gpu, labels, H, W, False, dist0, 5, C, D=dist0 + W, **ann)
            assert status == INVALID and _untouched(obs, sd, cd), (where, index, value)
            if inside:
                status, obs, sd, cd = _call(gpu, labels, H, W, False, dist0, 5, C, d_min=cut, d_lo=cut, D=3, **ann)
                assert status == INVALID and _untouched(obs, sd, cd), (where, index, value)
            else:
                want = R.tables(labels, H, W, False, dist0, 5, C, d_min=cut, d_lo=cut, D=3, **good)
                _check(gpu, labels, H, W, False, dist0, 5, C, d_min=cut, ref=want, **ann)
    row = good["row_class"].copy()                           # a diagonal block: the one array serves rows and columns
    row[7] = C
    sq = _map("blocky", H, H, True, 5, 2)
    status, obs, sd, cd = _call(gpu, sq, H, H, True, 0, 5, C, row, d_min=0, d_max=0, D=1)
    assert status == INVALID and _untouched(obs, sd, cd)


# ---- argument refusals ------------------------------------------------------------------------------------------------------
def test_refused_arguments_write_nothing(gpu):
    lab = np.zeros(64, dtype=np.uint8)
    big = np.zeros(65536, dtype=np.uint8)
    seg = np.zeros(8, dtype=np.int32)
    ok = dict(labels=lab, H=4, W=5, diag=False, dist0=0, K=3, C=2, row_class=np.zeros(4), col_class=np.zeros(5), D=5)
    assert _call(gpu, **ok)[0] == 0
    assert _call(gpu, **dict(ok, row_seg=seg, col_seg=seg))[0] == 0
    cases = [
        (dict(null=("labels",)), INVALID), (dict(null=("row_class",)), INVALID), (dict(null=("obs",)), INVALID),
        (dict(null=("state_dist",)), INVALID), (dict(null=("cat_dist",)), INVALID),
        (dict(null=("col_class",)), INVALID),                # an off-diagonal block needs column classes
        (dict(row_seg=seg), INVALID), (dict(col_seg=seg), INVALID),            # one segment array without the other
        (dict(H=0), INVALID), (dict(W=0), INVALID), (dict(H=-2), INVALID), (dict(K=0), INVALID), (dict(K=-1), INVALID),
        (dict(C=0), INVALID), (dict(C=-1), INVALID), (dict(D=-1), INVALID),
        (dict(diag=True), INVALID),                          # 4 x 5: not square
        (dict(diag=True, W=4, dist0=1), INVALID),            # a diagonal block with dist0 != 0
        (dict(diag=True, W=4, dist0=-1), INVALID),
        (dict(d_min=-1), INVALID), (dict(d_min=3, d_max=2), INVALID), (dict(d_min=0, d_max=-2), INVALID),
        (dict(D=4), INVALID),                                # the distances are 0 .. 4
        (dict(d_lo=1, D=5), INVALID), (dict(D=0), INVALID), (dict(d_min=2, d_max=3, d_lo=3, D=1), INVALID),
        (dict(d_min=2, d_max=3, d_lo=2, D=1), INVALID), (dict(dist0=-2, d_lo=1, D=9), INVALID),   # -5 .. 2: the distance 0 is there
        (dict(K=65), UNSUPPORTED), (dict(C=9), UNSUPPORTED),
        (dict(diag=True, H=65536, W=65536, row_class=big, small=True), UNSUPPORTED),          # n = 2^31 + 2^15
        (dict(H=46341, W=46341, row_class=big, col_class=big, small=True), UNSUPPORTED),      # n = 2,147,488,281
        (dict(dist0=(1 << 31) - 9, small=True), UNSUPPORTED),                    # |dist0| + H + W = 2^31
        (dict(dist0=-((1 << 31) - 9), small=True), UNSUPPORTED),
        (dict(dist0=1 << 40, small=True), UNSUPPORTED),
        (dict(K=64, D=1 << 25, small=True), UNSUPPORTED),                       # D K = 2^31
        (dict(C=8, D=1 << 24, small=True), UNSUPPORTED),                        # D 2 C C = 2^31
        (dict(D=1 << 31, small=True), UNSUPPORTED),
    ]
    for change, want in cases:
        status, obs, sd, cd = _call(gpu, **dict(ok, **change))
        assert status == want, change
        assert _untouched(obs, sd, cd), change
    # a table that starts below the window and ends above it, a window that nothing reaches with D == 0, and a diagonal block
    # without column arrays and with row segments alone
    assert _call(gpu, **dict(ok, d_min=2, d_max=3, d_lo=1, D=4))[0] == 0
    assert _call(gpu, **dict(ok, d_min=9, D=0))[0] == 0
    status, obs, _, _ = _call(gpu, **dict(ok, diag=True, W=4, D=4, col_class=None, row_seg=seg))
    assert status == 0 and obs.sum() == 10 and obs[1].sum() == 10           # class 0 with itself, all inside segment 0


def test_huge_window_bounds_are_no_error(gpu):
    labels = _map("random", 40, 50, False, 4, 1)
    ann = _annotation(40, 50, False, 2, 1)
    _check(gpu, labels, 40, 50, False, 2, 4, 2, d_min=0, d_max=1 << 40, **ann)                 # as good as no upper limit
    for d_min, d_max in ((1 << 40, -1), (1 << 40, 1 << 41)):                                   # nothing inside
        status, obs, sd, cd = _call(gpu, labels, 40, 50, False, 2, 4, 2, d_min=d_min, d_max=d_max, d_lo=7, D=2, **ann)
        assert status == 0 and not obs.any() and not sd.any() and not cd.any()


# ---- other properties -------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes(gpu):
    for H, W, diag in ((300, 300, True), (100, 600, False)):
        labels = _map("random", H, W, diag, 20, 4)
        ann = _annotation(H, W, diag, 3, 5, "per_bin")
        d_lo, D = enrich.distance_range(H, W, diag, 0, 1, 280)
        a = _call(gpu, labels, H, W, diag, 0, 20, 3, d_min=1, d_max=280, d_lo=d_lo, D=D, **ann)
        b = _call(gpu, labels, H, W, diag, 0, 20, 3, d_min=1, d_max=280, d_lo=d_lo, D=D, **ann)
        assert a[0] == 0 and b[0] == 0 and a[1].any()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def test_cat_dist_does_not_depend_on_the_labels(gpu):
    H, W = 90, 310
    ann = _annotation(H, W, False, 4, 6)
    got = [_check(gpu, _map(kind, H, W, False, 11, 8), H, W, False, 12, 11, 4, d_min=4, d_max=200, **ann) for kind in ("blocky", "random")]
    assert np.array_equal(got[0][2], got[1][2]) and not np.array_equal(got[0][0], got[1][0])


def test_one_class_without_segments_is_the_contingency_diagonal(gpu):
    from phylo_hmrf_amd import compare
    H, W, K = 90, 310, 11
    labels = _map("blocky", H, W, False, K, 8)
    obs, sd, _ = _check(gpu, labels, H, W, False, 12, K, 1, np.zeros(H, dtype=np.uint8), np.zeros(W, dtype=np.uint8))
    assert np.array_equal(obs[0], np.diagonal(compare.contingency(labels, labels, K, K))) and not obs[1].any()
    assert np.array_equal(obs[0], sd.sum(axis=0))


# ---- end to end -------------------------------------------------------------------------------------------------------------
K_GENOME, C_GENOME = 6, 3
# per chromosome a diagonal region and the off-diagonal region beside it
SHAPES = [(70, 70, 1, 0, 0, 1), (70, 45, 0, 0, 90, 1), (33, 33, 1, 4, 4, 2), (33, 20, 0, 4, 50, 2)]


def _genome(paint=None):
    """-> (state_vec, len_vec, bin_class, bin_seg).  The states are a function of the distance alone; paint = (class, state):
    the bin pairs of that class inside one segment take that state instead."""
    rng = np.random.default_rng(77)
    bin_class = {1: _intervals(rng, 120, 0, C_GENOME).astype(np.uint8), 2: _intervals(rng, 70, 0, C_GENOME).astype(np.uint8)}
    bin_seg = {1: np.repeat(np.arange(40), 4)[:120].astype(np.int32), 2: np.repeat(np.arange(100, 120), 5)[:70].astype(np.int32)}
    bin_seg[1][rng.random(120) < 0.2] = -1
    parts, rows, at = [], [], 0
    for r, (H, W, diag, s1, s2, chrom) in enumerate(SHAPES):
        i, j = R.nodes(H, W, bool(diag))
        lab = (np.abs(s2 - s1 + j - i) // 3) % (K_GENOME - 1)
        if paint is not None:
            cls, seg = np.zeros(200, dtype=np.int64), np.full(200, -1, dtype=np.int64)
            cls[:len(bin_class[chrom])], seg[:len(bin_seg[chrom])] = bin_class[chrom], bin_seg[chrom]
            hit = (cls[s1 + i] == paint[0]) & (cls[s2 + j] == paint[0]) & (seg[s1 + i] >= 0) & (seg[s1 + i] == seg[s2 + j])
            lab = np.where(hit, paint[1], lab)
        parts.append(lab.astype(np.uint8))
        rows.append([lab.size, at, at + lab.size, H, W, s1, s2, r, diag, chrom])
        at += lab.size
    return np.concatenate(parts), np.array(rows, dtype=np.int64), bin_class, bin_seg


def test_pair_enrichment_end_to_end():
    s, L, bin_class, bin_seg = _genome()
    rng = np.random.default_rng(3)
    noisy = np.where(rng.random(s.size) < 0.3, rng.integers(0, K_GENOME, s.size), s)
    for window in ((0, -1), (2, 60), (500, -1)):
        for segs in (bin_seg, None):
            got = enrich.pair_enrichment(noisy, L, bin_class, segs, window=window, K=K_GENOME, C=C_GENOME)
            ref = R.pair_enrichment(noisy, L, bin_class, segs, window, K_GENOME, C_GENOME)
            for name in ("obs", "obs_region", "state_dist", "cat_dist"):
                assert got[name].dtype == np.int64 and got[name].shape == ref[name].shape, (name, window)
                assert np.array_equal(got[name], ref[name]), (name, window)
            assert int(got["d0"]) == ref["d0"] and got["window"].tolist() == list(window)
            assert np.allclose(got["expected"], ref["expected"], rtol=1e-12, atol=1e-9)
            n = got["obs"].sum()
            assert np.max(np.abs(got["expected"].sum(axis=1) - got["obs"].sum(axis=1))) <= 1e-9 * max(n, 1)
            assert np.max(np.abs(got["expected"].sum(axis=0) - got["obs"].sum(axis=0))) <= 1e-9 * max(n, 1)
    # the arrays of chromosome 1 end at bin 120 of 135, chromosome 2 has none at all: class 0, no segment
    got = enrich.pair_enrichment(noisy.reshape(1, -1).astype(np.float64), L, {1: bin_class[1]}, {1: bin_seg[1]}, C=C_GENOME)
    ref = R.pair_enrichment(noisy, L, {1: bin_class[1]}, {1: bin_seg[1]}, (0, -1), K_GENOME, C_GENOME)
    assert int(got["K"]) == K_GENOME and int(got["C"]) == C_GENOME and np.array_equal(got["obs_region"], ref["obs_region"])
    assert int(enrich.pair_enrichment(noisy, L, {2: bin_class[2]})["C"]) == int(bin_class[2].max()) + 1 == C_GENOME
    assert got["obs_region"][2:].reshape(2, -1, K_GENOME)[:, 1:].sum() == 0
    with pytest.raises(RuntimeError):
        enrich.pair_enrichment(noisy, L, bin_class, K=3)     # a state >= K inside the window
    with pytest.raises(RuntimeError):
        enrich.pair_enrichment(noisy, L, bin_class, C=2)     # a class >= C inside the window


def test_a_distance_only_map_is_enriched_nowhere():
    s, L, bin_class, bin_seg = _genome()
    got = enrich.pair_enrichment(s, L, bin_class, bin_seg, K=K_GENOME, C=C_GENOME)
    held = got["expected"] > 0
    assert np.array_equal(got["expected"], got["obs"].astype(np.float64)) and held.any() and not held.all()
    assert np.all(got["log2_enrichment"][held] == np.log2(1.0 + 1e-16)) and np.all(np.isnan(got["log2_enrichment"][~held]))


def test_a_painted_category_is_the_largest_enrichment():
    cls, state = 2, K_GENOME - 1
    s, L, bin_class, bin_seg = _genome(paint=(cls, state))
    got = enrich.pair_enrichment(s, L, bin_class, bin_seg, K=K_GENOME, C=C_GENOME)
    p = (cls * C_GENOME + cls) * 2 + 1
    assert got["obs"][p, state] > 0 and got["obs"][:, state].sum() == got["obs"][p, state] == got["obs"][p].sum()
    assert np.unravel_index(np.nanargmax(got["log2_enrichment"]), got["log2_enrichment"].shape) == (p, state)


def test_enrich_files_round_trip(tmp_path):
    import scipy.io
    s, L, _, _ = _genome()
    path = os.path.join(str(tmp_path), "estimate_ou_7.mat")
    scipy.io.savemat(path, dict(state_vec=s.reshape(1, -1), state_vec_smooth=(5 - s).reshape(1, -1), len_vec=L))
    bed = os.path.join(str(tmp_path), "tads.bed")
    with open(bed, "w") as fh:
        fh.write("#chrom start stop name\nchr1 0 1000000 A\nchr1 1000000 3000000 B\nchr1 2500000 5000000 A\nchrX 0 5 A\n"
                 "chr2 200000 2600000 B\n")
    out = enrich.enrich_files(path, bed, str(tmp_path / "out"), 50000, field="state_vec_smooth", window_bp="100000-3000000",
                              segments=True)
    assert os.path.basename(out) == "enrich_estimate_ou_7.npz"
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["enrich_estimate_ou_7.npz", "enrich_estimate_ou_7.txt"]
    z = np.load(out, allow_pickle=False)
    ann = enrich.read_annotation(bed, L, 50000, segments=True)
    assert ann["names"] == ["none", "A", "B"] and ann["skipped_lines"] == 1 and z["names"].tolist() == ann["names"]
    ref = R.pair_enrichment(5 - s, L, ann["bin_class"], ann["bin_seg"], (2, 60), 6, 3)
    for name in ("obs", "obs_region", "state_dist", "cat_dist"):
        assert np.array_equal(z[name], ref[name]), name
    assert z["window"].tolist() == [2, 60] and int(z["d0"]) == ref["d0"] and np.array_equal(z["len_vec"], L)
    assert int(z["resolution"]) == 50000 and str(z["enrich_field"]) == "state_vec_smooth" and int(z["segments"]) == 1
    assert str(z["window_bp"]) == "100000-3000000" and int(z["skipped_lines"]) == 1 and int(z["C"]) == 3 and int(z["K"]) == 6
    assert np.array_equal(z["class_1"], ann["bin_class"][1]) and np.array_equal(z["seg_2"], ann["bin_seg"][2])
    lines = open(os.path.join(str(tmp_path / "out"), "enrich_estimate_ou_7.txt")).read().splitlines()
    assert lines[0] == enrich.HEADER
    cells = [ln.split("\t") for ln in lines[1:]]
    folded = enrich.fold_pairs(ref["obs"], 3)
    assert len(cells) == 6 * int((folded.sum(axis=3) > 0).sum()) and all(len(c) == 9 for c in cells)
    names = ann["names"]
    for c in cells:
        a, b, same, k = names.index(c[0]), names.index(c[1]), int(c[2]), int(c[3]) - 1
        assert a <= b and int(c[4]) == folded[a, b, same, k]
    assert sum(int(c[4]) for c in cells) == ref["obs"].sum()
