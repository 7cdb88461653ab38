"""GPU: a state map resampled onto another grid (phmrf_regrid_states, phylo_hmrf_amd.regrid) against the restatement of
tests/regrid_reference.py, which loops over target cells and source cells as the definition reads.  Everything is integer
arithmetic: every comparison is exact.  Every output is filled with a pattern before the call, so an entry the call did not
write shows and a refused call is seen to write nothing."""
import ctypes
import os

import numpy as np
import pytest

from phylo_hmrf_amd import regrid
from tests import regrid_reference as R

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4
FILL = 0xA5
LAYOUT_A = [(7, 7, 0, 0, 1, 1), (12, 12, 7, 7, 1, 1), (7, 12, 0, 7, 0, 1)]      # two diagonal blocks and the block between them
LAYOUT_B = [(19, 19, 0, 0, 1, 1)]
ODD = [(1, 1, 0, 0, 1, 2)]                                   # one node of another chromosome in front: every slice starts at an odd byte


@pytest.fixture(scope="module")
def gpu():
    import torch
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    return L, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _nodes(H, W, diag):
    return H * (H + 1) // 2 if diag else H * W


def _regions(L, chrom):
    rows = L[L[:, 9] == chrom]
    return np.ascontiguousarray(rows[:, [1, 3, 4, 5, 6, 8]], dtype=np.int64)


def _call(gpu, s, regs, target, a, b, K, min_cover, fill=None, want=(True, True), null=(), R_given=None, n_labels=None):
    """One phmrf_regrid_states call for the target (H, W, start_bin1, start_bin2, diagonal) -> (status, state, support, covered,
    hist, mixed); the outputs hold FILL before the call.  want: pass support_dev, covered_dev; null: names passed as NULL."""
    import torch
    lib, dev, st = gpu
    H, W, t1, t2, diag = target
    n_t = max(1, _nodes(max(H, 1), max(W, 1), diag if diag in (0, 1) else 0)) if H < 70000 else 1
    s_t = torch.from_numpy(np.asarray(s).astype(np.uint8)).to(dev)
    state = torch.full((n_t,), FILL, dtype=torch.uint8, device=dev)
    support = torch.full((n_t,), -0x5A5A5A5B, dtype=torch.int32, device=dev)           # 0xA5A5A5A5
    covered = torch.full((n_t,), -0x5A5A5A5B, dtype=torch.int32, device=dev)
    hist = np.full(K + 1 if K >= 1 else 1, -0x5A5A5A5A5A5A5A5B, dtype=np.int64)
    mixed = ctypes.c_int64(-0x5A5A5A5A5A5A5A5B)
    regs = np.ascontiguousarray(regs, dtype=np.int64)
    ptr = lambda name, p: None if name in null else p
    status = lib.phmrf_regrid_states(ptr("labels", ctypes.c_void_p(s_t.data_ptr())), len(s) if n_labels is None else n_labels,
                                     regs.shape[0] if R_given is None else R_given,
                                     ptr("regions", regs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), K, a, b, H, W, diag, t1, t2,
                                     min_cover, K if fill is None else fill, ptr("state", ctypes.c_void_p(state.data_ptr())),
                                     ctypes.c_void_p(support.data_ptr()) if want[0] else None,
                                     ctypes.c_void_p(covered.data_ptr()) if want[1] else None,
                                     ptr("hist", hist.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
                                     ptr("mixed", ctypes.byref(mixed)), st)
    torch.cuda.synchronize()
    return (status, state.cpu().numpy(), support.cpu().numpy().view(np.uint32), covered.cpu().numpy().view(np.uint32), hist,
            int(mixed.value))


def _untouched(out):
    _, state, support, covered, hist, mixed = out
    return (np.all(state == FILL) and np.all(support == 0xA5A5A5A5) and np.all(covered == 0xA5A5A5A5) and
            np.all(hist == -0x5A5A5A5A5A5A5A5B) and mixed == -0x5A5A5A5A5A5A5A5B)


def _check(gpu, s, L, chrom, target, a, b, K, min_cover=1):
    """the call against the reference, everything equal -> the call's outputs"""
    H, W, t1, t2, diag = target
    C, bad = R.planes(s, L, chrom, K)
    w_state, w_support, w_covered, w_hist, w_mixed = R.regrid_region(C, bad, a, b, H, W, diag, t1, t2, min_cover, K)
    out = _call(gpu, s, _regions(L, chrom), target, a, b, K, min_cover)
    status, state, support, covered, hist, mixed = out
    assert status == 0, regrid_error(gpu)
    assert np.array_equal(state, w_state), np.nonzero(state != w_state)[0][:10]
    assert np.array_equal(support, w_support) and np.array_equal(covered, w_covered)
    assert np.array_equal(hist, w_hist) and mixed == w_mixed
    assert int(hist.sum()) == _nodes(H, W, diag)
    return out


def regrid_error(gpu):
    return gpu[0].phmrf_last_error().decode()


def _expected_sparse(C, bad, a, b, H, W, diag, t1, t2, min_cover, K):
    """R.regrid_region's five results with its cell loop made only over the target cells whose source rectangle holds a node
    (told by an integral image of the occupied source cells): a cell that reads nothing has no votes, so it is uncalled with
    support = covered = 0.  For targets far larger than the map."""
    B = C.shape[1]
    S = np.zeros((B + 1, B + 1), dtype=np.int64)
    S[1:, 1:] = ((C.sum(axis=0) > 0) | bad).cumsum(axis=0).cumsum(axis=1)

    def span(t, n):
        x = t + np.arange(n, dtype=np.int64)
        return np.minimum(B, (x * b) // a), np.minimum(B, -(-((x + 1) * b) // a))
    (p0, p1), (q0, q1) = span(t1, H), span(t2, W)
    held = S[np.ix_(p1, q1)] - S[np.ix_(p0, q1)] - S[np.ix_(p1, q0)] + S[np.ix_(p0, q0)]
    state, support, covered = np.full((H, W), K, dtype=np.uint8), np.zeros((H, W), dtype=np.uint32), np.zeros((H, W), dtype=np.uint32)
    for i, j in np.argwhere(held > 0):
        if diag and i > j:
            continue
        votes = R.cell_votes(C, bad, a, b, t1 + int(i), t2 + int(j))
        k = int(np.argmax(votes))
        support[i, j], covered[i, j] = votes[k], votes.sum()
        if covered[i, j] >= min_cover:
            state[i, j] = k
    pick = (lambda x: x[np.triu_indices(H)]) if diag else (lambda x: x.reshape(-1))
    state, support, covered = pick(state), pick(support), pick(covered)
    return state, support, covered, np.bincount(state, minlength=K + 1).astype(np.int64), int(np.sum((state != K) & (support < covered)))


def _check_second_trip(gpu, s, L, target, a, b, K, first_trip):
    """a target of more cells than one trip of the kernel's grid takes, far larger than the map, against _expected_sparse; the
    cells of the second trip and the cells the same lanes (waves) took before them must both hold mixed cells"""
    H, W, t1, t2, diag = target
    C, bad = R.planes(s, L, 1, K)
    want = _expected_sparse(C, bad, a, b, H, W, diag, t1, t2, 1, K)
    mixed = (want[0] != K) & (want[1] < want[2])
    n_t = _nodes(H, W, diag)
    assert first_trip < n_t <= 2 * first_trip and np.any(mixed[first_trip:] & mixed[:n_t - first_trip])
    out = _call(gpu, s, _regions(L, 1), target, a, b, K, 1)
    assert out[0] == 0, regrid_error(gpu)
    for got, exp in zip(out[1:5], want[:4]):
        assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    assert out[5] == want[4]


def _map(layout, B, K, seed, blocky=False, front=ODD):
    L = R.len_vec_of(front + layout)
    return R.state_vec_of(L, {1: R.symmetric(B, K, seed, blocky), 2: np.zeros((1, 1), dtype=np.int64)}), L


# ---- re-layout at a = b = 1 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("front", [[], ODD])
def test_relayout(gpu, front):
    K = 6
    sa, LA = _map(LAYOUT_A, 19, K, 1, front=front)
    sb, LB = _map(LAYOUT_B, 19, K, 1, front=front)
    out = _check(gpu, sa, LA, 1, (19, 19, 0, 0, 1), 1, 1, K)
    assert np.array_equal(out[1], sb[len(front):]) and np.all(out[2] == 1) and np.all(out[3] == 1) and out[5] == 0
    at = len(front)
    for (H, W, s1, s2, diag, _) in LAYOUT_A:                 # and the inverse, region by region
        out = _check(gpu, sb, LB, 1, (H, W, s1, s2, diag), 1, 1, K)
        n = _nodes(H, W, diag)
        assert np.array_equal(out[1], sa[at:at + n])
        at += n


# ---- integer coarsening and refining ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocky", [False, True])
def test_coarsen_by_5(gpu, blocky):
    K = 20
    s, L = _map([(53, 53, 0, 0, 1, 1)], 53, K, 2, blocky)
    out = _check(gpu, s, L, 1, (11, 11, 0, 0, 1), 1, 5, K)   # the last row and column are partly covered
    assert out[3][10] == 15 and out[3][-1] == 9 and out[3][0] == 25
    _check(gpu, s, L, 1, (11, 11, 0, 0, 1), 1, 5, K, min_cover=13)
    _check(gpu, s, L, 1, (5, 9, 3, 2, 0), 1, 5, K)           # a target start that is no multiple of 5, below and across the diagonal
    s, L = _map([(20, 20, 3, 3, 1, 1), (30, 30, 23, 23, 1, 1), (20, 30, 3, 23, 0, 1)], 53, K, 3, blocky)
    _check(gpu, s, L, 1, (11, 11, 0, 0, 1), 1, 5, K)         # source regions that start and meet inside target bins
    _check(gpu, s, L, 1, (7, 7, 3, 3, 1), 1, 5, K, min_cover=25)


def test_refine_by_5(gpu):
    K = 5
    s, L = _map(LAYOUT_A, 19, K, 4)
    out = _check(gpu, s, L, 1, (95, 95, 0, 0, 1), 5, 1, K)
    assert np.all(out[3] == 1)
    _check(gpu, s, L, 1, (33, 41, 13, 47, 0), 5, 1, K)
    _check(gpu, s, L, 1, (20, 20, 88, 88, 1), 5, 1, K)       # past the end of the map


# ---- rational ratios --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(2, 5), (5, 2), (3, 7)])
def test_rational_ratios(gpu, a, b):
    K = 7
    s, L = _map([(20, 20, 3, 3, 1, 1), (30, 30, 23, 23, 1, 1), (20, 30, 3, 23, 0, 1)], 53, K, 5, blocky=True)
    side = -(-53 * a // b)
    _check(gpu, s, L, 1, (side, side, 0, 0, 1), a, b, K)
    _check(gpu, s, L, 1, (side - 1, side - 1, 1, 1, 1), a, b, K, min_cover=regrid.min_cover_of(50, b))   # a start inside a source bin
    _check(gpu, s, L, 1, (5, 7, 1, 4, 0), a, b, K)
    _check(gpu, s, L, 1, (6, 4, 5, 2, 0), a, b, K, min_cover=b * b)


# ---- large ratio and the threshold between the two kernels -------------------------------------------------------------------
def test_large_ratio(gpu):
    K = 9
    assert not regrid.is_small(1, 40)
    s, L = _map([(80, 80, 0, 0, 1, 1), (120, 120, 80, 80, 1, 1), (80, 120, 0, 80, 0, 1)], 200, K, 6, blocky=True)
    _check(gpu, s, L, 1, (5, 5, 0, 0, 1), 1, 40, K)
    _check(gpu, s, L, 1, (2, 3, 3, 1, 0), 1, 40, K, min_cover=800)


@pytest.mark.parametrize("b", [16, 17])
def test_either_side_of_the_small_area(gpu, b):
    K = 12
    assert regrid.max_bins(1, 16) ** 2 == regrid.SMALL_AREA and regrid.is_small(1, b) == (b == 16)
    s, L = _map([(40, 40, 0, 0, 1, 1), (60, 60, 40, 40, 1, 1), (40, 60, 0, 40, 0, 1)], 100, K, 7, blocky=True)
    _check(gpu, s, L, 1, (7, 7, 0, 0, 1), 1, b, K)
    _check(gpu, s, L, 1, (3, 4, 3, 1, 0), 1, b, K, min_cover=b * b // 2)


@pytest.mark.parametrize("b", [regrid.ROW_W, regrid.ROW_W + 1, regrid.ROW_W + 14])
def test_rows_at_and_beyond_a_row_piece(gpu, b):
    """the wave kernel walks a storage row in pieces of ROW_W columns: a target cell ROW_W source bins wide (one piece for
    its widest rows), one more (a second piece of one column) and 14 more"""
    K = 4
    s, L = _map([(300, 300, 0, 0, 1, 1)], 300, K, 8, blocky=True, front=ODD)
    _check(gpu, s, L, 1, (2, 2, 0, 0, 1), 1, b, K)


# ---- more target cells than one trip of a kernel's grid ------------------------------------------------------------------------
def test_sparse_reference_is_the_reference():
    K = 5
    s, L = _map([(20, 20, 3, 3, 1, 1), (30, 30, 23, 23, 1, 1), (20, 30, 3, 23, 0, 1)], 53, K, 21, blocky=True, front=[])
    C, bad = R.planes(s, L, 1, K)
    for target, a, b, min_cover in (((14, 14, 1, 1, 1), 1, 5, 13), ((9, 40, 6, 0, 0), 2, 5, 1), ((30, 12, 20, 110, 0), 5, 2, 4)):
        H, W, t1, t2, diag = target
        want = R.regrid_region(C, bad, a, b, H, W, diag, t1, t2, min_cover, K)
        got = _expected_sparse(C, bad, a, b, H, W, diag, t1, t2, min_cover, K)
        assert all(np.array_equal(x, y) for x, y in zip(got[:4], want[:4])) and got[4] == want[4]


def test_lane_kernel_second_trip(gpu):
    """GRID_CAP workgroups of LANES cells take 524,288 target cells a trip.  A 730 x 730 target at b = 2 over two strips of 24 source
    rows 1,436 bins apart: target rows 0 - 11 (first trip) and 718 - 729 (second trip, the same lanes 148 columns further
    on) hold mixed cells, as do the columns of the strips' mirror images; everything between reads nothing."""
    K = 4
    L = R.len_vec_of(ODD + [(24, 1360, 0, 100, 0, 1), (24, 1300, 1436, 100, 0, 1)])
    s = np.random.default_rng(22).integers(0, K, int(L[-1, 2]))
    _check_second_trip(gpu, s, L, (730, 730, 0, 0, 0), 1, 2, K, regrid.GRID_CAP * regrid.LANES)


def test_wave_kernel_second_trip(gpu):
    """WAVE_GRID_CAP workgroups of WAVES waves take 8,192 target cells a trip.  A 92 x 92 target at b = 17 over a block of rows
    0 - 50 x columns 1400 - 1499 and a diagonal block of bins 1500 - 1599: the cells (0 .. 2, 84 .. 87) of the first trip and
    (89 .. 91, 88 .. 91) of the second go to the same waves."""
    K = 3
    assert not regrid.is_small(1, 17)
    L = R.len_vec_of(ODD + [(51, 100, 0, 1400, 0, 1), (100, 100, 1500, 1500, 1, 1)])
    s = np.random.default_rng(23).integers(0, K, int(L[-1, 2]))
    _check_second_trip(gpu, s, L, (92, 92, 0, 0, 0), 1, 17, K, regrid.WAVE_GRID_CAP * regrid.WAVES)


# ---- mirror and seam cases --------------------------------------------------------------------------------------------------
def test_mirrors_seams_and_nothing(gpu):
    K = 6
    s, L = _map(LAYOUT_A, 19, K, 9)
    _check(gpu, s, L, 1, (6, 5, 12, 1, 0), 1, 1, K)          # below the diagonal: covered only through mirror images
    _check(gpu, s, L, 1, (3, 2, 4, 0, 0), 1, 3, K)
    _check(gpu, s, L, 1, (8, 9, 2, 5, 0), 1, 1, K)           # across the seam of the three regions
    _check(gpu, s, L, 1, (4, 5, 1, 1, 0), 2, 3, K)
    out = _check(gpu, s, L, 1, (4, 6, 30, 40, 0), 1, 1, K)   # no source region reaches it
    assert np.all(out[1] == K) and out[4][K] == 24 and not out[3].any()
    out = _check(gpu, s, L, 1, (5, 5, 25, 25, 1), 1, 2, K)
    assert np.all(out[1] == K) and out[4][K] == 15


# ---- tile edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [regrid.LANES + 1, 2 * regrid.LANES + 3])
def test_one_row_of_a_tile_and_a_bit(gpu, W):
    K = 8
    s, L = _map([(262, 262, 0, 0, 1, 1)], 262, K, 10, blocky=True)
    _check(gpu, s, L, 1, (1, W, 100, 2, 0), 1, 1, K)
    _check(gpu, s, L, 1, (1, W, 0, 1, 0), 2, 1, K)           # refining: 131 and 260 source bins wide


def test_a_diagonal_target_one_wider_than_a_tile(gpu):
    K = 8
    s, L = _map([(262, 262, 0, 0, 1, 1)], 262, K, 11, blocky=True)
    _check(gpu, s, L, 1, (regrid.LANES + 1, regrid.LANES + 1, 0, 0, 1), 1, 2, K)


# ---- K extremes and ties ----------------------------------------------------------------------------------------------------
def test_k_extremes_and_ties(gpu):
    s, L = _map(LAYOUT_A, 19, 1, 12)
    out = _check(gpu, s, L, 1, (4, 4, 0, 0, 1), 1, 5, 1)
    assert np.all(out[1] == 0) and out[5] == 0
    s, L = _map(LAYOUT_A, 19, 64, 13)
    s[1:5] = [63, 0, 63, 62]
    out = _check(gpu, s, L, 1, (10, 10, 0, 0, 1), 1, 2, 64)
    assert out[4][64] == 0 and np.all(out[1] < 64)           # every cell called
    out = _check(gpu, s, L, 1, (19, 19, 0, 0, 1), 1, 1, 64)
    assert out[4][64] == 0
    # the 4-bin map of tests/test_regrid_cpu.py: two 2 x 2 equal splits, the lowest state wins
    s4 = np.array([1, 0, 2, 2, 1, 0, 3, 3, 1, 3])
    L4 = R.len_vec_of([(4, 4, 0, 0, 1, 1)])
    out = _check(gpu, s4, L4, 1, (2, 2, 0, 0, 1), 1, 2, 4)
    assert out[1].tolist() == [0, 2, 1] and out[2].tolist() == [2, 2, 2] and out[3].tolist() == [4, 4, 4] and out[5] == 3


def test_k_extremes_and_a_tie_through_the_wave_kernel(gpu):
    assert not regrid.is_small(1, 17) and not regrid.is_small(1, 18)
    s, L = _map(LAYOUT_A, 19, 1, 24)
    out = _check(gpu, s, L, 1, (2, 2, 0, 0, 1), 1, 17, 1)
    assert np.all(out[1] == 0) and out[5] == 0
    M = R.symmetric(36, 64, 25)
    M[0:9, 18:36], M[9:18, 18:36] = 63, 62                   # target cell (0, 1) at b = 18: 162 votes each, the lowest state wins
    M[18:36, 0:18] = M[0:18, 18:36].T
    M = np.triu(M) + np.triu(M, 1).T
    L = R.len_vec_of(ODD + [(36, 36, 0, 0, 1, 1)])
    s = R.state_vec_of(L, {1: M, 2: np.zeros((1, 1), dtype=np.int64)})
    out = _check(gpu, s, L, 1, (2, 2, 0, 0, 1), 1, 18, 64)
    assert out[1][1] == 62 and out[2][1] == 162 and out[3][1] == 324 and out[4][64] == 0


# ---- the call threshold -----------------------------------------------------------------------------------------------------
def test_covered_equal_to_min_cover_is_called(gpu):
    K = 5
    s, L = _map([(53, 53, 0, 0, 1, 1)], 53, K, 14)
    at_15 = _check(gpu, s, L, 1, (11, 11, 0, 0, 0), 1, 5, K, min_cover=15)
    at_16 = _check(gpu, s, L, 1, (11, 11, 0, 0, 0), 1, 5, K, min_cover=16)
    edge = at_15[3] == 15                                    # the last row and column without the corner
    assert edge.sum() == 20 and np.all(at_15[1][edge] < K) and np.all(at_16[1][edge] == K)
    assert at_15[4][K] == 1 and at_16[4][K] == 21


# ---- inspection and refusals ------------------------------------------------------------------------------------------------
def test_a_label_above_k_counts_only_where_it_is_read(gpu):
    K = 6
    s, L = _map(LAYOUT_A, 19, K, 15)
    regs = _regions(L, 1)
    bad = s.copy()
    bad[1 + 0] = 200                                         # bin pair (0, 0)
    _check(gpu, bad, L, 1, (3, 3, 1, 1, 1), 1, 5, K)         # bins 5 .. 19: not read
    _check(gpu, bad, L, 1, (9, 9, 1, 1, 1), 1, 2, K)
    for target, a, b in (((4, 4, 0, 0, 1), 1, 5), ((1, 1, 0, 0, 0), 1, 1), ((2, 2, 0, 0, 1), 1, 17)):
        out = _call(gpu, bad, regs, target, a, b, K, 1)
        assert out[0] == INVALID and _untouched(out) and ">= K" in regrid_error(gpu)
    bad = s.copy()
    bad[-1] = K                                              # the last node of the off-diagonal block: (6, 18), read through the mirror
    out = _call(gpu, bad, regs, (1, 1, 18, 6, 0), 1, 1, K, 1)
    assert out[0] == INVALID and _untouched(out)
    assert _call(gpu, bad, regs, (1, 1, 18, 5, 0), 1, 1, K, 1)[0] == 0


def test_refusals(gpu):
    K = 6
    s, L = _map(LAYOUT_A, 19, K, 16)
    regs = _regions(L, 1)
    T = (4, 4, 0, 0, 1)

    def refused(status, text="", **kw):
        args = dict(s=s, regs=regs, target=T, a=1, b=5, K=K, min_cover=1)
        args.update(kw)
        out = _call(gpu, **args)
        assert out[0] == status, (kw, out[0], regrid_error(gpu))
        assert _untouched(out), kw
        assert text in regrid_error(gpu), (kw, regrid_error(gpu))

    assert _call(gpu, s, regs, T, 1, 5, K, 1)[0] == 0
    for name in ("labels", "regions", "state", "hist", "mixed"):
        refused(INVALID, "NULL", null=(name,))
    refused(INVALID, n_labels=0)
    refused(INVALID, R_given=0)
    refused(INVALID, K=0)
    refused(INVALID, a=0)
    refused(INVALID, b=0)
    refused(INVALID, "min_cover", min_cover=0)
    refused(INVALID, "min_cover", min_cover=26)
    refused(INVALID, fill=256)
    refused(INVALID, fill=-1)
    refused(INVALID, target=(0, 4, 0, 0, 0))
    refused(INVALID, target=(4, 0, 0, 0, 0))
    refused(INVALID, target=(4, 4, 0, 0, 2))
    refused(INVALID, target=(4, 5, 0, 0, 1))
    refused(INVALID, target=(4, 4, -1, 0, 0))
    refused(INVALID, "start_bin1 == start_bin2", target=(4, 4, 0, 1, 1))
    for col, value in ((1, 0), (2, 0), (0, -1), (0, len(s)), (3, -1), (4, -1), (5, 2)):      # a bad source region row
        bad = regs.copy()
        bad[2, col] = value
        refused(INVALID, regs=bad)
    bad = regs.copy()
    bad[1, 4] = 8                                            # a diagonal source region with unequal start bins
    refused(INVALID, "region 1", regs=bad)
    # overlap in its three forms
    bad = regs.copy()
    bad[1, 3:5] = 6
    refused(INVALID, "regions 0 and 1 overlap", regs=bad)
    bad = np.concatenate([regs, [[1, 2, 2, 11, 5, 0]]])     # rows 11 - 12 x columns 5 - 6: the mirror image of a part of region 2
    refused(INVALID, "regions 2 and 3 overlap through the mirror", regs=bad)
    bad = regs.copy()
    bad[2] = [1, 5, 5, 20, 24, 0]
    refused(INVALID, "region 2 overlaps its own mirror", regs=bad)
    # unsupported
    refused(UNSUPPORTED, K=65)
    refused(UNSUPPORTED, regs=np.concatenate([regs] * 22)[:65])
    refused(UNSUPPORTED, a=(1 << 15) + 1)
    refused(UNSUPPORTED, b=(1 << 15) + 1)
    refused(UNSUPPORTED, target=(4, 4, 1 << 30, 1 << 30, 1))
    refused(UNSUPPORTED, target=(70000, 70000, 0, 0, 0))
    bad = regs.copy()
    bad[2, 4] = 1 << 30
    refused(UNSUPPORTED, regs=bad)
    bad = regs.copy()
    bad[2, 1:3] = 70000
    refused(UNSUPPORTED, regs=bad)
    assert _call(gpu, s, regs, T, 1 << 15, 1 << 15, K, 1 << 30)[0] == 0       # the largest a, b and min_cover


# ---- output options and determinism -----------------------------------------------------------------------------------------
def test_null_planes_and_the_same_bytes_twice(gpu):
    K = 9
    s, L = _map([(80, 80, 0, 0, 1, 1), (120, 120, 80, 80, 1, 1), (80, 120, 0, 80, 0, 1)], 200, K, 17)
    regs = _regions(L, 1)
    for target, a, b in (((67, 67, 0, 0, 1), 1, 3), ((5, 5, 0, 0, 1), 1, 40)):
        full = _call(gpu, s, regs, target, a, b, K, 1)
        again = _call(gpu, s, regs, target, a, b, K, 1)
        assert full[0] == 0 and all(np.array_equal(x, y) for x, y in zip(full[1:5], again[1:5])) and full[5] == again[5]
        bare = _call(gpu, s, regs, target, a, b, K, 1, want=(False, False))
        assert bare[0] == 0 and np.array_equal(bare[1], full[1]) and np.array_equal(bare[4], full[4]) and bare[5] == full[5]
        assert np.all(bare[2] == 0xA5A5A5A5) and np.all(bare[3] == 0xA5A5A5A5)
        half = _call(gpu, s, regs, target, a, b, K, 1, want=(False, True))
        assert np.all(half[2] == 0xA5A5A5A5) and np.array_equal(half[3], full[3])


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_regrid_states_over_two_chromosomes():
    K = 7
    L = R.len_vec_of(LAYOUT_A + [(9, 9, 0, 0, 1, 3)])
    s = R.state_vec_of(L, {1: R.symmetric(19, K, 18, True), 3: R.symmetric(9, K, 19)})
    D = R.len_vec_of([(4, 4, 0, 0, 1, 1), (3, 3, 0, 0, 1, 2), (2, 4, 0, 1, 0, 1), (2, 2, 0, 0, 1, 3)])   # chromosome 2: not in the source
    got = regrid.regrid_states(s, L, 10000, D, 50000, K=K, cover=50)
    want = R.regrid(s, L, D, 1, 5, K, 13)
    for name in ("state_vec", "support", "covered", "hist_region", "mixed_region"):
        assert np.array_equal(got[name], want[name]), name
    assert got["state_vec"].dtype == np.uint8 and got["support"].dtype == np.uint32 and got["covered"].dtype == np.uint32
    assert np.all(got["state_vec"][10:16] == K) and got["hist_region"][1].tolist() == [0] * K + [6]
    assert (int(got["K"]), int(got["fill"]), int(got["a"]), int(got["b"]), int(got["min_cover"])) == (K, K, 1, 5, 13)
    called = got["state_vec"] != K
    assert np.array_equal(got["conf"][called], (want["support"][called] / want["covered"][called]).astype(np.float32))
    assert not got["conf"][~called].any() and np.array_equal(got["cover"], (want["covered"] / 25.0).astype(np.float32))
    with pytest.raises(ValueError):                          # overlapping source regions
        regrid.regrid_states(s, R.len_vec_of([(7, 7, 0, 0, 1, 1), (12, 12, 6, 6, 1, 1)]), 10000, D, 50000)
    with pytest.raises(RuntimeError):                        # a state >= K inside a read cell
        regrid.regrid_states(s, L, 10000, D, 50000, K=2)
    s64 = s.copy()
    s64[0] = 63
    with pytest.raises(ValueError):                          # K = 64 and an uncalled cell
        regrid.regrid_states(s64, L, 10000, D, 50000)
    assert regrid.regrid_states(s64, L, 10000, D[:1], 50000, cover=0)["hist_region"][0, 64] == 0


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_command_line_regrid_then_compare(tmp_path):
    import scipy.io
    import phylo_hmrf as cli
    K, f = 5, 5
    LB = R.len_vec_of(LAYOUT_B)
    M = R.symmetric(19, K, 20, blocky=True)
    sb = R.state_vec_of(LB, {1: M})
    LA = R.len_vec_of([(7 * f, 7 * f, 0, 0, 1, 1), (12 * f, 12 * f, 7 * f, 7 * f, 1, 1), (7 * f, 12 * f, 0, 7 * f, 0, 1)])
    sa = R.state_vec_of(LA, {1: np.kron(M, np.ones((f, f), dtype=np.int64))})
    LB = np.concatenate([LB, [[123]]], axis=1)               # an 11th column, as a loader may write: copied verbatim
    a_mat, b_mat, out = str(tmp_path / "A.mat"), str(tmp_path / "B.mat"), str(tmp_path / "out")
    scipy.io.savemat(a_mat, {"state_vec": sa, "len_vec": LA})
    scipy.io.savemat(b_mat, {"state_vec": sb, "len_vec": LB})
    base = ["10", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1", "0.5", "8", "0",
            "0.001", "0", "1", "test", "0", "0", "60", "50000", "1", "hg38", out]
    path = cli.run(*base, regrid=a_mat, regrid_from="10000", regrid_like=b_mat)
    assert path == os.path.join(out, "regrid_A_50000.mat") and os.path.exists(os.path.join(out, "regrid_A_50000.txt"))
    d = scipy.io.loadmat(path)
    assert np.array_equal(d["state_vec"].reshape(-1), sb) and np.array_equal(d["len_vec"], LB)
    assert np.all(d["covered"] == 25) and np.all(d["conf"] == 1) and int(d["uncovered_state"].reshape(-1)[0]) == -1
    assert np.array_equal(d["src_len_vec"], LA)
    cmp_path = cli.run(*base, compare=path, compare_with=b_mat)
    assert float(scipy.io.loadmat(cmp_path)["agreement"].reshape(-1)[0]) == 1.0
