"""GPU: the enrichment's permutation null (phmrf_pair_enrichment_null, phylo_hmrf_amd.enrich.enrichment_null) against the
restatement of tests/enrich_null_reference.py: rolled chromosome arrays, tests/enrich_reference.tables per shift and the
fixed-point expectation in Python integers.  Everything is integer arithmetic: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

from phylo_hmrf_amd import enrich
from tests import enrich_null_reference as N
from tests import enrich_reference as R

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4
FILL = 0xA5
ONE = 1 << 24
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


def _call(gpu, labels, H, W, diag, row0, col0, K, C, cls, seg, B, shifts, w, d_min=0, d_max=-1, d_lo=0, D=0, offset=0, null=(),
          small=False, T=None):
    """-> (status, obs int64 [T, 2 C C, K], expq int64 [T, 2 C C, K]); both buffers are filled with FILL before the call.  The
    labels start `offset` bytes into their device buffer.  null: names of pointers passed as NULL.  small: a call that must
    be refused, with one-word buffers.  T: the count passed, where it is not len(shifts)."""
    import torch
    L, dev, st = gpu
    shifts = np.ascontiguousarray(shifts, dtype=np.int32)
    T = len(shifts) if T is None else T
    k, c, t = max(K, 1), max(C, 1), max(T, 1)
    P = 2 * c * c
    obs, exq = (_filled(1 if small else t * P * k) for _ in range(2))
    a = np.zeros(offset + len(labels), dtype=np.uint8)
    a[offset:] = labels
    held = [torch.from_numpy(a).to(dev)[offset:]]

    def up(name, x, dtype):
        if x is None or name in null:
            return None
        held.append(torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(dev))
        return ctypes.c_void_p(held[-1].data_ptr())

    w = np.ascontiguousarray(w, dtype=np.uint32)
    out = lambda name, x: None if name in null else x.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    status = L.phmrf_pair_enrichment_null(
        None if "labels" in null else ctypes.c_void_p(held[0].data_ptr()), H, W, int(diag), row0, col0, K, C, up("cls", cls, np.uint8),
        up("seg", seg, np.int32), B, None if "shifts" in null else shifts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), T, d_min,
        d_max, d_lo, D, None if "weights" in null else w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), out("obs", obs),
        out("expq", exq), st)
    if not small and status == 0:
        obs, exq = obs.reshape(t, P, k), exq.reshape(t, P, k)
    return status, obs, exq


def _weights(D, K, seed):
    """any weights will do: the call's expq is exact for every table of entries <= ONE; 0 and ONE themselves occur"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, ONE + 1, (D, K)).astype(np.uint32)
    w[rng.random((D, K)) < 0.2] = 0
    w[rng.random((D, K)) < 0.2] = ONE
    return w


def _check(gpu, labels, H, W, diag, row0, col0, K, C, cls, seg, B, shifts, d_min=0, d_max=-1, offset=0, what="", w=None):
    """the call on the tight table range against the restatement"""
    rng = enrich.distance_range(H, W, diag, col0 - row0, d_min, d_max)
    d_lo, D = (d_min, 0) if rng is None else rng
    w = _weights(D, K, H + W + len(shifts)) if w is None else w
    status, obs, exq = _call(gpu, labels, H, W, diag, row0, col0, K, C, cls, seg, B, shifts, w, d_min, d_max, d_lo, D, offset)
    what = (what, H, W, diag, row0, col0, K, C, B, d_min, d_max, offset)
    assert status == 0, what
    want = N.tables(labels, H, W, diag, row0, col0, K, C, cls, seg, B, shifts, w.astype(np.int64), d_min, d_max, d_lo, D)
    for name, got, ref in zip(("obs", "expq"), (obs, exq), want):
        assert got.shape == ref.shape and np.array_equal(got, ref), (what, name, np.argwhere(got != ref)[:5].tolist())
    return obs, exq


# ---- maps and annotations ---------------------------------------------------------------------------------------------------
def _map(kind, H, W, diag, K, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        M = rng.integers(0, K, (H, W))
    else:                                                    # blocky: constant tiles of 1 - 9 rows by 1 - 9 columns
        rows = np.repeat(np.arange(H), rng.integers(1, 10, H))[:H]
        cols = np.repeat(np.arange(W), rng.integers(1, 10, W))[:W]
        M = rng.integers(0, K, (H, W))[rows][:, cols]
    return (M[np.triu_indices(H)] if diag else M.reshape(-1)).astype(np.uint8)


def _intervals(rng, n, lo, hi, longest=20):
    lengths = rng.integers(1, longest + 1, n + 1)
    return np.repeat(rng.integers(lo, hi, lengths.shape[0]), lengths)[:n]


SEGMENTS = ("absent", "given", "all_none")


def _chromosome(B, C, seed, segments="given", longest=20):
    """-> (classes u8 [B], segments int32 [B] or None): intervals of 1 .. longest bins, few segment ids so that bins far apart
    meet in one segment"""
    rng = np.random.default_rng(seed)
    cls = _intervals(rng, B, 0, C, longest).astype(np.uint8)
    if segments == "absent":
        return cls, None
    return cls, (_intervals(rng, B, -1, 6, longest).astype(np.int32) if segments == "given" else np.full(B, -1, dtype=np.int32))


def _seam_shifts(H, W, row0, col0, B):
    """0, 1, B - 1 and the shifts that put the wrap seam inside the first tile's rows and columns, inside the second's, and
    exactly on the tile bounds"""
    out = [0, 1, B - 1]
    for start, size, bound in ((row0, H, enrich.TILE_H), (col0, W, enrich.TILE_W)):
        for at in (5, bound, bound + 5, 2 * bound, size - 1):            # the region's bin `at` is the first one past the seam
            if 0 < at < size:
                out.append((B - start - at) % B)
    return sorted({s for s in out if 0 <= s < B})


# ---- shapes, seams and windows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, 2, 33, 129, 257])
def test_diagonal_blocks(gpu, side):
    """B = side: the seam falls inside the region under every shift but 0; B = side + 40: the region in the middle"""
    K, C = 20, 3
    labels = _map("random", side, side, True, K, side)
    for B, row0 in ((side, 0), (side + 40, 20)):
        cls, seg = _chromosome(B, C, side + B)
        shifts = _seam_shifts(side, side, row0, row0, B)
        for d_min, d_max in WINDOWS:
            obs, _ = _check(gpu, labels, side, side, True, row0, row0, K, C, cls, seg, B, shifts, d_min, d_max)
            if (d_min, d_max) == (0, -1):
                assert (obs.sum(axis=(1, 2)) == side * (side + 1) // 2).all()              # stored nodes count once, under every shift


@pytest.mark.parametrize("H,W", [(1, 7), (7, 1), (65, 130), (257, 300)])
def test_off_diagonal_blocks(gpu, H, W):
    K, C = 20, 3
    labels = _map("random", H, W, False, K, H * 1000 + W)
    for row0, col0, tail in ((0, H + 3, 0), (W + 10, 0, 0), (20, 20 + H // 2, 40), (5, 5 + W + 60, 20)):
        B = max(row0 + H, col0 + W) + tail
        cls, seg = _chromosome(B, C, H + W + B)
        shifts = _seam_shifts(H, W, row0, col0, B)
        near = (max(0, abs(col0 - row0) - 2), abs(col0 - row0) + 20)
        for d_min, d_max in WINDOWS + (near,):
            obs, _ = _check(gpu, labels, H, W, False, row0, col0, K, C, cls, seg, B, shifts, d_min, d_max)
            if (d_min, d_max) == (0, -1):
                assert (obs.sum(axis=(1, 2)) == H * W).all()


def test_rows_and_columns_far_apart_on_a_long_chromosome(gpu):
    H, W, row0, col0, B = 40, 150, 1000, 300000, 300500
    labels = _map("blocky", H, W, False, 7, 3)
    cls, seg = _chromosome(B, 4, 8, longest=400)
    shifts = [0, 1, B - 1, B - col0 - 30, B - row0 - 7, 123456, B - col0 - W + 1]
    obs, _ = _check(gpu, labels, H, W, False, row0, col0, 7, 4, cls, seg, B, shifts)
    assert (obs.sum(axis=(1, 2)) == H * W).all()
    _check(gpu, labels, H, W, False, row0, col0, 7, 4, cls, seg, B, shifts, col0 - row0 - 10, col0 - row0 + 25)


def _tile_windows():
    out = []
    for bound in (enrich.TILE_H, enrich.TILE_W):
        for b in (bound - 1, bound, bound + 1):
            out += [(b, -1), (0, b), (b, b)]
    out.append((enrich.TILE_H, enrich.TILE_W))
    return out


@pytest.mark.parametrize("H,W,diag,row0,col0", [(2 * enrich.TILE_W + 8, 2 * enrich.TILE_W + 8, True, 9, 9),
                                                (2 * enrich.TILE_H + 6, enrich.TILE_W + 3, False, enrich.TILE_H + 4, 4)])
def test_windows_at_the_tile_bounds(gpu, H, W, diag, row0, col0):
    """tiles wholly outside the window (not read), wholly inside it (no per-cell test) and cut by it lie side by side"""
    B = max(row0 + H, col0 + W) + 11
    labels = _map("blocky", H, W, diag, 20, H + W)
    cls, seg = _chromosome(B, 3, H)
    shifts = [0, B - row0 - enrich.TILE_H, B - col0 - enrich.TILE_W - 3]
    for d_min, d_max in _tile_windows():
        _check(gpu, labels, H, W, diag, row0, col0, 20, 3, cls, seg, B, shifts, d_min, d_max)


# ---- K, C and the groups of shifts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 8])
@pytest.mark.parametrize("K", [1, 2, 20, 64])
def test_state_and_class_counts(gpu, K, C):
    """T = 1, one full group and one group and a shift (K = 64, C = 8, the largest LDS configuration: T = 3 with groups of ONE
    shift, and the expectation kernel's states in two slices); segments absent, given and all -1 in turn"""
    ts = enrich.null_group(K, C)
    for m, (H, W, diag, row0, col0) in enumerate(((130, 130, True, 3, 3), (65, 130, False, 0, 72))):
        B = col0 + W + 9
        labels = _map(("random", "blocky")[m], H, W, diag, K, K + m)
        for n_shifts in ((3,) if ts == 1 else (1, ts, ts + 1)):
            segments = SEGMENTS[(m + n_shifts + K) % 3]
            cls, seg = _chromosome(B, C, 10 * m + n_shifts, segments, longest=(1, 20)[(m + n_shifts) % 2])
            shifts = np.random.default_rng(n_shifts).integers(0, B, n_shifts)
            for d_min, d_max in ((0, -1), (3, 17)):
                _check(gpu, labels, H, W, diag, row0, col0, K, C, cls, seg, B, shifts, d_min, d_max, what=(segments, n_shifts))


def test_three_groups_of_shifts(gpu):
    K, C = 64, 4
    ts = enrich.null_group(K, C)
    assert ts == 6
    H, W, B = 70, 140, 260
    labels = _map("blocky", H, W, False, K, 1)
    cls, seg = _chromosome(B, C, 2)
    shifts = np.random.default_rng(5).integers(0, B, 3 * ts)
    obs, exq = _check(gpu, labels, H, W, False, 10, 100, K, C, cls, seg, B, shifts)
    assert len({o.tobytes() for o in obs}) == 3 * ts           # (every shift its own table)


@pytest.mark.parametrize("segments", SEGMENTS)
def test_segments(gpu, segments):
    for H, W, diag, row0, col0 in ((130, 130, True, 0, 0), (65, 130, False, 0, 20)):
        B = col0 + W
        labels = _map("blocky", H, W, diag, 20, 5)
        cls, seg = _chromosome(B, 4, 7, segments)
        obs, _ = _check(gpu, labels, H, W, diag, row0, col0, 20, 4, cls, seg, B, [0, 11, B - 1], what=segments)
        inside = obs.reshape(3, 4, 4, 2, 20)[:, :, :, 1].sum(axis=(1, 2, 3))
        assert ((inside > 0) == (segments == "given")).all()


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_label_slices_start_at_any_byte(gpu, offset):
    for H, W, diag, row0, col0 in ((65, 65, True, 2, 2), (63, 65, False, 0, 70), (5, 300, False, 1, 0), (9, 3, False, 0, 4)):
        B = max(row0 + H, col0 + W) + 6
        cls, seg = _chromosome(B, 3, H)
        labels = _map("random", H, W, diag, 20, offset + H)
        _check(gpu, labels, H, W, diag, row0, col0, 20, 3, cls, seg, B, [0, 3, B - 2], offset=offset)
        _check(gpu, labels, H, W, diag, row0, col0, 20, 3, cls, seg, B, [0, 3, B - 2], 2, 40, offset=offset)


# ---- the grid strides and a long distance axis ------------------------------------------------------------------------------
def test_more_tiles_than_the_grid_cap(gpu):
    """T = 2: one group, so the counting kernel's workgroups stride over the tiles, and the expectation kernel's over the
    diagonals"""
    H, W, K, C = 16500, 129, 3, 2
    assert -(-H // enrich.TILE_H) * -(-W // enrich.TILE_W) > enrich.NULL_GRID_CAP and enrich.null_group(K, C) >= 2
    assert (H + W - 1) * -(-min(H, W) // enrich.NULL_CHUNK) > 4 * (enrich.NULL_CLASS_CAP // 2)
    B = H + 200
    labels = _map("blocky", H, W, False, K, 3)
    cls, seg = _chromosome(B, C, 8, longest=300)
    obs, _ = _check(gpu, labels, H, W, False, 0, 150, K, C, cls, seg, B, [B - 7000, 11])
    assert (obs.sum(axis=(1, 2)) == H * W).all()


def test_a_long_distance_axis(gpu):
    """D = 8,200 distances, 2 categories and T = 2,049 shifts: T D P > 2^25 entries, where a stored table of the categories
    per shift and distance would pass 128 MiB.  (The expectation is fused: no such table is stored, so there is no scratch
    whose chunks a call could be cut into; the size stays as the case that would have needed two.)"""
    H, W, B, T = 1, 8200, 8300, 2049
    assert T * (H + W - 1) * 2 > 1 << 25
    labels = _map("random", H, W, False, 2, 1)
    cls, _ = _chromosome(B, 1, 1, "absent")
    shifts = np.random.default_rng(2).integers(0, B, T)
    _check(gpu, labels, H, W, False, 50, 60, 2, 1, cls, None, B, shifts)


# ---- cross-checks -----------------------------------------------------------------------------------------------------------
def test_shift_zero_is_the_enrichment_itself(gpu):
    from tests.test_gpu_enrich import _call as enrich_call
    for H, W, diag, row0, col0 in ((150, 150, True, 12, 12), (90, 140, False, 4, 130)):
        B, K, C = col0 + W + 5, 9, 3
        labels = _map("blocky", H, W, diag, K, 2)
        cls, seg = _chromosome(B, C, 4)
        for d_min, d_max in ((0, -1), (4, 60)):
            d_lo, D = enrich.distance_range(H, W, diag, col0 - row0, d_min, d_max)
            status, obs1, sd, cd = enrich_call(gpu, labels, H, W, diag, col0 - row0, K, C, cls[row0:row0 + H], cls[col0:col0 + W],
                                               seg[row0:row0 + H], seg[col0:col0 + W], d_min, d_max, d_lo, D)
            assert status == 0
            w = enrich.weights(sd)
            status, obs, exq = _call(gpu, labels, H, W, diag, row0, col0, K, C, cls, seg, B, [0, 9], w, d_min, d_max, d_lo, D)
            assert status == 0 and np.array_equal(obs[0], obs1) and np.array_equal(exq[0], enrich.expected_fixed(cd, w))
            assert not np.array_equal(obs[1], obs1)
            # the fixed-point expectation under the float one, by at most 2^-24 bin pairs per bin pair of the category
            gap = enrich.expected(sd, cd) * ONE - exq[0]
            assert np.all(gap >= -1e-9 * ONE * cd.sum()) and np.all(gap <= cd.sum(axis=0)[:, None] + 1e-9 * ONE * cd.sum())


def test_two_calls_give_equal_bytes_and_obs_ignores_the_weights(gpu):
    for H, W, diag, row0, col0 in ((300, 300, True, 0, 0), (100, 600, False, 0, 50)):
        B = col0 + W + 30
        labels = _map("random", H, W, diag, 20, 4)
        cls, seg = _chromosome(B, 3, 5, longest=1)
        d_lo, D = enrich.distance_range(H, W, diag, col0 - row0, 1, 280)
        shifts = np.random.default_rng(1).integers(0, B, 20)
        w = _weights(D, 20, 1)
        a = _call(gpu, labels, H, W, diag, row0, col0, 20, 3, cls, seg, B, shifts, w, 1, 280, d_lo, D)
        b = _call(gpu, labels, H, W, diag, row0, col0, 20, 3, cls, seg, B, shifts, w, 1, 280, d_lo, D)
        c = _call(gpu, labels, H, W, diag, row0, col0, 20, 3, cls, seg, B, shifts, _weights(D, 20, 2), 1, 280, d_lo, D)
        z = _call(gpu, labels, H, W, diag, row0, col0, 20, 3, cls, seg, B, shifts, np.zeros((D, 20)), 1, 280, d_lo, D)
        assert a[0] == b[0] == c[0] == z[0] == 0 and a[1].any() and a[2].any()
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        assert a[1].tobytes() == c[1].tobytes() == z[1].tobytes() and a[2].tobytes() != c[2].tobytes() and not z[2].any()


# ---- bad labels and classes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,diag,row0,col0", [(70, 70, True, 6, 6), (40, 300, False, 0, 3)])
def test_bad_label_inside_and_outside_the_window(gpu, H, W, diag, row0, col0):
    dist0, B = col0 - row0, col0 + W + 8
    good = _map("random", H, W, diag, 5, 9)
    cls, seg = _chromosome(B, 3, 1)
    i, j = 2, 33
    d = abs(dist0 + j - i)
    at = i * W - i * (i - 1) // 2 + (j - i) if diag else i * W + j
    shifts = [0, 5, B - 1]
    for bad_state in (5, 64, 255):
        labels = good.copy()
        labels[at] = bad_state
        for d_min, d_max in ((0, -1), (d, d), (0, d), (d, -1)):
            d_lo, D = enrich.distance_range(H, W, diag, dist0, d_min, d_max)
            status, obs, exq = _call(gpu, labels, H, W, diag, row0, col0, 5, 3, cls, seg, B, shifts, _weights(D, 5, 1), d_min, d_max, d_lo, D)
            assert status == INVALID and _untouched(obs, exq), (bad_state, d_min, d_max)
        for d_min, d_max in ((0, d - 1), (d + 1, -1), (d + 1, d + 1)):
            d_lo, D = enrich.distance_range(H, W, diag, dist0, d_min, d_max)
            w = _weights(D, 5, 2)
            want = N.tables(good, H, W, diag, row0, col0, 5, 3, cls, seg, B, shifts, w.astype(np.int64), d_min, d_max, d_lo, D)
            status, obs, exq = _call(gpu, labels, H, W, diag, row0, col0, 5, 3, cls, seg, B, shifts, w, d_min, d_max, d_lo, D)
            assert status == 0 and np.array_equal(obs, want[0]) and np.array_equal(exq, want[1]), (bad_state, d_min, d_max)


def test_a_bad_class_that_only_a_shift_brings_inside(gpu):
    H, W, C, K = 40, 40, 3, 5
    B, row0 = H + 40, 20
    labels = _map("blocky", H, W, True, K, 2)
    good, seg = _chromosome(B, C, 3)
    w = _weights(H, K, 3)
    for value in (C, 255):
        cls = good.copy()
        cls[row0 + H + 4] = value                            # four bins past the region: shifts 5 .. 44 bring it inside
        assert _call(gpu, labels, H, W, True, row0, row0, K, C, cls, seg, B, [0, 4, 45, B - 1], w, D=H)[0] == 0
        _check(gpu, labels, H, W, True, row0, row0, K, C, cls, seg, B, [0, 4, 45, B - 1], w=w)
        for s in (5, 44, 20):
            status, obs, exq = _call(gpu, labels, H, W, True, row0, row0, K, C, cls, seg, B, [0, s, 1], w, D=H)
            assert status == INVALID and _untouched(obs, exq), (value, s)
        # under the shift 44 the bad bin is the region's bin 0: its nodes have the distances 0 .. 39, (0, 39) alone the last
        assert _call(gpu, labels, H, W, True, row0, row0, K, C, cls, seg, B, [44], w[39:], 39, -1, 39, 1)[0] == INVALID
        cls[row0 + H + 4], cls[row0 + 1] = good[row0 + H + 4], value       # bin 1: outside the window (39, -1) unshifted
        assert _call(gpu, labels, H, W, True, row0, row0, K, C, cls, seg, B, [0], w[39:], 39, -1, 39, 1)[0] == 0
        assert _call(gpu, labels, H, W, True, row0, row0, K, C, cls, seg, B, [0, 1], w[39:], 39, -1, 39, 1)[0] == INVALID
        assert _call(gpu, labels, H, W, True, row0, row0, K, C, cls, seg, B, [0], w, D=H)[0] == INVALID


# ---- argument refusals ------------------------------------------------------------------------------------------------------
def test_refused_arguments_write_nothing(gpu):
    """(T 2 C C K >= 2^26 cannot be reached through the entry point: T <= 4096, C <= 8 and K <= 64 give at most 2^25; the
    command line's N reaches it, tests/test_enrich_null_cpu.py)"""
    lab = np.zeros(64, dtype=np.uint8)
    seg = np.zeros(20, dtype=np.int32)
    ok = dict(labels=lab, H=4, W=5, diag=False, row0=2, col0=2, K=3, C=2, cls=np.zeros(20), seg=None, B=20, shifts=[0, 19],
              w=np.full((5, 3), ONE), D=5)
    status, obs, exq = _call(gpu, **ok)
    assert status == 0 and obs.sum() == 40 and exq.sum() == 40 * 3 * ONE
    assert _call(gpu, **dict(ok, seg=seg))[0] == 0
    many = np.zeros(4097, dtype=np.int32)
    cases = [
        (dict(null=("labels",)), INVALID), (dict(null=("cls",)), INVALID), (dict(null=("shifts",)), INVALID),
        (dict(null=("weights",)), INVALID), (dict(null=("obs",)), INVALID), (dict(null=("expq",)), INVALID),
        (dict(diag=2), INVALID), (dict(diag=-1), INVALID),
        (dict(diag=True), INVALID),                          # 4 x 5: not square
        (dict(diag=True, W=4, col0=3), INVALID),             # a diagonal block with row0 != col0
        (dict(H=0), INVALID), (dict(W=0), INVALID), (dict(K=0), INVALID), (dict(C=0), INVALID), (dict(D=-1), INVALID),
        (dict(row0=-1), INVALID), (dict(col0=-1), INVALID), (dict(row0=17), INVALID), (dict(col0=16), INVALID), (dict(B=6), INVALID),
        (dict(shifts=[0, 20]), INVALID), (dict(shifts=[-1]), INVALID), (dict(shifts=[3, 1 << 30]), INVALID),
        (dict(shifts=[], T=0), INVALID), (dict(T=-1), INVALID),
        (dict(w=np.full((5, 3), ONE + 1)), INVALID), (dict(w=np.array([[0] * 14 + [1 << 31]])), INVALID),
        (dict(d_min=-1), INVALID), (dict(d_min=3, d_max=2), INVALID), (dict(d_min=0, d_max=-2), INVALID),
        (dict(D=4), INVALID), (dict(d_lo=1, D=5), INVALID), (dict(D=0), INVALID),              # the distances are 0 .. 4
        (dict(K=65, small=True), UNSUPPORTED), (dict(C=9, small=True), UNSUPPORTED),
        (dict(shifts=many, small=True), UNSUPPORTED),                                          # T = 4097
        (dict(B=1 << 31, small=True), UNSUPPORTED), (dict(B=1 << 40, row0=1 << 35, small=True), UNSUPPORTED),
        (dict(diag=True, H=65536, W=65536, B=1 << 20, small=True), UNSUPPORTED),               # n = 2^31 + 2^15
        (dict(H=46341, W=46341, B=1 << 20, small=True), UNSUPPORTED),
        (dict(K=64, D=1 << 25, small=True), UNSUPPORTED), (dict(D=1 << 31, small=True), UNSUPPORTED),
    ]
    for change, want in cases:
        status, obs, exq = _call(gpu, **dict(ok, **change))
        assert status == want, change
        assert _untouched(obs, exq), change
    # a window that nothing reaches gives zeros, whatever the table; a table wider than the window needs is fine
    status, obs, exq = _call(gpu, **dict(ok, d_min=9, D=0, w=np.zeros((0, 3))))
    assert status == 0 and not obs.any() and not exq.any() and obs.shape == (2, 8, 3)
    assert _call(gpu, **dict(ok, d_min=2, d_max=3, d_lo=1, D=4, w=np.full((4, 3), 7)))[0] == 0
    assert _call(gpu, **dict(ok, shifts=np.zeros(4096, dtype=np.int32)))[0] == 0               # T = 4096 is served


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _genome_shifts(T=99, seed=11):
    rng = np.random.default_rng(seed)
    return {1: rng.integers(5, 131, T).astype(np.int64), 2: rng.integers(5, 66, T).astype(np.int64)}      # B = 135 and 70


@pytest.fixture(scope="module")
def noisy():
    from tests.test_gpu_enrich import _genome, K_GENOME
    s, L, bin_class, bin_seg = _genome()
    rng = np.random.default_rng(3)
    return np.where(rng.random(s.size) < 0.3, rng.integers(0, K_GENOME, s.size), s), L, bin_class, bin_seg


@pytest.mark.parametrize("window", [(0, -1), (2, 60)])
def test_enrichment_null_end_to_end(noisy, window):
    from tests.test_gpu_enrich import K_GENOME, C_GENOME
    s, L, bin_class, bin_seg = noisy
    shifts = _genome_shifts()
    for segs in (bin_seg, None):
        got = enrich.enrichment_null(s, L, bin_class, segs, window=window, K=K_GENOME, C=C_GENOME, shifts=shifts)
        ref = N.genome(s, L, bin_class, segs, window, K_GENOME, C_GENOME, shifts)
        base = enrich.pair_enrichment(s, L, bin_class, segs, window=window, K=K_GENOME, C=C_GENOME)
        for name in base:                                    # pair_enrichment's dict, unchanged
            assert np.array_equal(got[name], base[name], equal_nan=base[name].dtype.kind == "f"), name
        assert got["weights"].dtype == np.uint32 and np.array_equal(got["weights"], ref["weights"])
        for name in ("expq", "null_obs", "null_expq"):
            assert got[name].dtype == np.int64 and got[name].shape == ref[name].shape and np.array_equal(got[name], ref[name]), name
        assert got["null_obs"].shape == (99, 2 * C_GENOME * C_GENOME, K_GENOME)
        assert sorted(got["shifts"]) == [1, 2] and all(np.array_equal(got["shifts"][c], shifts[c]) for c in shifts)
        want = enrich.null_statistics(ref["obs"], ref["expq"], ref["null_obs"], ref["null_expq"], C_GENOME)
        for name in enrich.STATISTICS:
            assert got[name].shape == (C_GENOME, C_GENOME, 2, K_GENOME) and np.array_equal(got[name], want[name], equal_nan=True), name
        assert (got["null_obs"].sum(axis=(1, 2)) == got["obs"].sum()).all()
        if segs is bin_seg:                                  # the calls cut into chunks of shifts: the same tables
            cut = enrich.enrichment_null(s, L, bin_class, segs, window=window, K=K_GENOME, C=C_GENOME, shifts=shifts, _max_call=40)
            assert all(cut[k].tobytes() == got[k].tobytes() for k in ("null_obs", "null_expq", "expq", "z", "p"))


def test_enrichment_null_draws_and_refuses(noisy):
    from tests.test_gpu_enrich import K_GENOME, C_GENOME
    s, L, bin_class, bin_seg = noisy
    a = enrich.enrichment_null(s, L, bin_class, bin_seg, n=17, min_shift=10, seed=5)
    b = enrich.enrichment_null(s, L, bin_class, bin_seg, n=17, min_shift=10, seed=5)
    drawn = enrich.draw_shifts(L, 17, min_shift=10, seed=5)
    assert all(np.array_equal(a["shifts"][c], drawn[c]) for c in drawn) and a["null_obs"].shape[0] == 17
    assert a["null_obs"].tobytes() == b["null_obs"].tobytes() and a["null_expq"].tobytes() == b["null_expq"].tobytes()
    assert int(a["K"]) == K_GENOME and int(a["C"]) == C_GENOME
    ref = N.genome(s, L, bin_class, bin_seg, (0, -1), K_GENOME, C_GENOME, drawn)
    assert np.array_equal(a["null_obs"], ref["null_obs"]) and np.array_equal(a["null_expq"], ref["null_expq"])
    for bad in (dict(shifts={1: [1, 2], 2: [1]}), dict(shifts={1: [1]}), dict(shifts={1: [135], 2: [0]}), dict(shifts={1: [-1], 2: [0]}),
                dict(shifts={1: [], 2: []}), dict(shifts={1: [0.5], 2: [0.5]}), dict(n=0), dict(n=3, _max_call=0)):
        with pytest.raises(ValueError):
            enrich.enrichment_null(s, L, bin_class, bin_seg, **bad)
    with pytest.raises(RuntimeError):
        enrich.enrichment_null(s, L, bin_class, bin_seg, C=2, n=3)           # a class >= C inside the window


def test_a_distance_only_map_has_no_excess_under_any_shift():
    from tests.test_gpu_enrich import _genome, K_GENOME, C_GENOME
    s, L, bin_class, bin_seg = _genome()
    got = enrich.enrichment_null(s, L, bin_class, bin_seg, K=K_GENOME, C=C_GENOME, shifts=_genome_shifts())
    assert np.array_equal(got["obs"] * ONE, got["expq"]) and np.array_equal(got["null_obs"] * ONE, got["null_expq"])
    assert got["null_obs"].any() and len({t.tobytes() for t in got["null_obs"]}) > 50
    assert not got["null_mean"].any() and not got["null_sd"].any() and np.isnan(got["z"]).all()
    assert (got["p"] == 1).all() and (got["p_high"] == 1).all() and (got["p_low"] == 1).all()


def test_a_painted_category_stands_out_of_its_null():
    from tests.test_gpu_enrich import _genome, K_GENOME, C_GENOME
    cls, state = 1, K_GENOME - 1
    s, L, bin_class, bin_seg = _genome(paint=(cls, state))
    got = enrich.enrichment_null(s, L, bin_class, bin_seg, K=K_GENOME, C=C_GENOME, shifts=_genome_shifts())
    print("painted: p_high %r z %r, the largest other z %r" % (got["p_high"][cls, cls, 1, state], got["z"][cls, cls, 1, state],
                                                               np.sort(got["z"][np.isfinite(got["z"])])[-2:].tolist()))
    assert got["obs"][(cls * C_GENOME + cls) * 2 + 1, state] > 0
    assert got["p_high"][cls, cls, 1, state] == 0.01
    assert np.unravel_index(np.nanargmax(got["z"]), got["z"].shape) == (cls, cls, 1, state)


def test_enrich_files_with_the_null_round_trip(tmp_path):
    import scipy.io
    from tests.test_gpu_enrich import _genome
    s, L, _, _ = _genome()
    path = os.path.join(str(tmp_path), "estimate_ou_7.mat")
    scipy.io.savemat(path, dict(state_vec=s.reshape(1, -1), state_vec_smooth=(5 - s).reshape(1, -1), len_vec=L))
    bed = os.path.join(str(tmp_path), "tads.bed")
    with open(bed, "w") as fh:
        fh.write("#chrom start stop name\nchr1 0 1000000 A\nchr1 1000000 3000000 B\nchr1 2500000 5000000 A\nchrX 0 5 A\n"
                 "chr2 200000 2600000 B\n")
    plain = enrich.enrich_files(path, bed, str(tmp_path / "plain"), 50000, field="state_vec_smooth", window_bp="100000-3000000",
                                segments=True)
    out = enrich.enrich_files(path, bed, str(tmp_path / "out"), 50000, field="state_vec_smooth", window_bp="100000-3000000",
                              segments=True, null=25, null_min_bp=500000, null_seed=4)
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["enrich_estimate_ou_7.npz", "enrich_estimate_ou_7.txt",
                                                         "enrich_estimate_ou_7_null.txt"]
    assert sorted(os.listdir(str(tmp_path / "plain"))) == ["enrich_estimate_ou_7.npz", "enrich_estimate_ou_7.txt"]
    z, z0 = np.load(out, allow_pickle=False), np.load(plain, allow_pickle=False)
    new = ["expq", "null_expq", "null_mean", "null_min_bp", "null_obs", "null_sd", "null_seed", "p", "p_high", "p_low", "shifts_1",
           "shifts_2", "weights", "z"]
    assert sorted(set(z.files) - set(z0.files)) == new and set(z0.files) <= set(z.files)
    for k in z0.files:                                       # what --enrich wrote it still writes
        assert z[k].tobytes() == z0[k].tobytes(), k
    text = lambda d, name: open(os.path.join(str(tmp_path / d), name), "rb").read()
    assert text("out", "enrich_estimate_ou_7.txt") == text("plain", "enrich_estimate_ou_7.txt")
    ann = enrich.read_annotation(bed, L, 50000, segments=True)
    drawn = enrich.draw_shifts(L, 25, min_shift=10, seed=4)
    assert all(np.array_equal(z["shifts_%d" % c], drawn[c]) for c in drawn) and int(z["null_seed"]) == 4
    ref = N.genome(5 - s, L, ann["bin_class"], ann["bin_seg"], (2, 60), 6, 3, drawn)
    for name in ("expq", "null_obs", "null_expq", "weights"):
        assert np.array_equal(z[name], ref[name]), name
    want = enrich.null_statistics(ref["obs"], ref["expq"], ref["null_obs"], ref["null_expq"], 3)
    assert all(np.array_equal(z[k], want[k], equal_nan=True) for k in enrich.STATISTICS)
    lines = text("out", "enrich_estimate_ou_7_null.txt").decode().splitlines()
    rows = text("out", "enrich_estimate_ou_7.txt").decode().splitlines()
    assert lines[0] == enrich.NULL_HEADER and len(lines) == len(rows) and all(len(ln.split("\t")) == 12 for ln in lines[1:])
    assert [ln.split("\t")[:5] for ln in lines[1:]] == [ln.split("\t")[:5] for ln in rows[1:]]


def test_the_command_line_writes_the_three_files(tmp_path):
    import scipy.io
    import phylo_hmrf as cli
    from tests.test_gpu_enrich import _genome
    s, L, _, _ = _genome()
    path = os.path.join(str(tmp_path), "estimate_ou_7.mat")
    scipy.io.savemat(path, dict(state_vec=s.reshape(1, -1), len_vec=L))
    bed = os.path.join(str(tmp_path), "tads.bed")
    with open(bed, "w") as fh:
        fh.write("chr1 0 1000000 A\nchr1 1000000 3000000 B\nchr1 2500000 5000000 A\nchr2 200000 2600000 B\n")
    out = cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1", "0.5", "8",
                  "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", str(tmp_path / "out"), quiet="1", enrich=path,
                  enrich_bed=bed, enrich_segments="1", enrich_null="7", enrich_null_min="250000", enrich_null_seed="3")
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["enrich_estimate_ou_7.npz", "enrich_estimate_ou_7.txt",
                                                         "enrich_estimate_ou_7_null.txt"]
    z = np.load(out, allow_pickle=False)
    drawn = enrich.draw_shifts(L, 7, min_shift=5, seed=3)
    assert z["null_obs"].shape == (7, 18, 5) and all(np.array_equal(z["shifts_%d" % c], drawn[c]) for c in drawn)
    assert int(z["null_min_bp"]) == 250000 and int(z["null_seed"]) == 3 and z["p"].shape == (3, 3, 2, 5)      # (the map holds the states 0 .. 4)
