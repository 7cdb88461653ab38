"""GPU: the rescaled pile-up of a state map over features of unequal size (phmrf_state_aggregate, phylo_hmrf_amd.aggregate)
against the restatement of tests/aggregate_reference.py, which loops over features, pile cells and stored nodes as the
definition reads.  Everything is integer arithmetic: every comparison is exact.  The host tables are filled with a pattern
before every call, so an entry the call did not write shows."""
import ctypes
import os

import numpy as np
import pytest

from phylo_hmrf_amd import aggregate, pileup, query
from tests import aggregate_reference as R

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4
FILL = 0xA5


@pytest.fixture(scope="module")
def gpu():
    import torch
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    return L, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- maps -------------------------------------------------------------------------------------------------------------------
def _len_vec(regions):
    """regions: (H, W, start_bin1, start_bin2, diagonal, chrom) -> len_vec int64 [R, 10], the nodes back to back"""
    rows, at = [], 0
    for r, (H, W, s1, s2, diag, chrom) in enumerate(regions):
        n = H * (H + 1) // 2 if diag else H * W
        rows.append([n, at, at + n, H, W, s1, s2, r, diag, chrom])
        at += n
    return np.array(rows, dtype=np.int64)


def _state_vec(L, matrices):
    """matrices: chrom -> the symmetric bin x bin matrix of the chromosome -> the stored nodes of every region of L"""
    parts = []
    for row in L:
        H, W, s1, s2, diag, chrom = (int(row[x]) for x in (3, 4, 5, 6, 8, 9))
        M = matrices[chrom][s1:s1 + H, s2:s2 + W]
        parts.append(M[np.triu_indices(H)] if diag else M.reshape(-1))
    return np.concatenate(parts).astype(np.int64)


def _symmetric(B, K, seed, blocky=False):
    rng = np.random.default_rng(seed)
    M = rng.integers(0, K, (B, B))
    if blocky:                                               # constant tiles of 1 - 9 bins a side: runs for the row walk
        cuts = np.repeat(np.arange(B), rng.integers(1, 10, B))[:B]
        M = M[cuts][:, cuts]
    return np.triu(M) + np.triu(M, 1).T


def _features(rows):
    return np.array(rows, dtype=np.int64).reshape(-1, 7)


# ---- the call ---------------------------------------------------------------------------------------------------------------
def _call(gpu, s, L, chrom, features, T, F, K, G, flip="given", small=False):
    """One phmrf_state_aggregate call for the features (already of `chrom`, any group order) -> (status, cells, votes); the
    tables are filled with FILL before the call and come back flat when it is refused.  flip None: a NULL pointer."""
    import torch
    lib, dev, st = gpu
    f = _features(features)
    f = f[np.argsort(f[:, 5], kind="stable")] if f.shape[0] else f
    offsets = np.concatenate([[0], np.cumsum(np.bincount(f[:, 5], minlength=G))]).astype(np.int64)
    regs = np.ascontiguousarray(L[L[:, 9] == chrom][:, [1, 3, 4, 5, 6, 8]], dtype=np.int64)
    P = max(T, 0) + 2 * max(F, 0)
    count = 1 if small else max(1, G * P * P * K)
    cells = np.full(8 * count, FILL, dtype=np.uint8).view(np.int64)
    votes = np.full(8 * count, FILL, dtype=np.uint8).view(np.int64)
    s_t = torch.from_numpy(np.asarray(s).astype(np.uint8)).to(dev)
    feat_t = torch.from_numpy(np.ascontiguousarray(f[:, 1:5], dtype=np.int32)).to(dev)
    flip_t = torch.from_numpy(np.ascontiguousarray(f[:, 6], dtype=np.uint8)).to(dev)
    i64 = ctypes.POINTER(ctypes.c_int64)
    status = lib.phmrf_state_aggregate(ctypes.c_void_p(s_t.data_ptr()), len(s), regs.shape[0], regs.ctypes.data_as(i64), K, T, F, G,
                                       offsets.ctypes.data_as(i64), ctypes.c_void_p(feat_t.data_ptr()) if f.shape[0] else None,
                                       None if flip is None else ctypes.c_void_p(flip_t.data_ptr()), cells.ctypes.data_as(i64),
                                       votes.ctypes.data_as(i64), st)
    if status == 0 and not small:
        cells, votes = cells.reshape(G, P, P, K), votes.reshape(G, P, P, K)
    return status, cells, votes


def _untouched(*tables):
    return all(bool(np.all(t.view(np.uint8) == FILL)) for t in tables)


def _check(gpu, s, L, features, T, F, K, G, what=""):
    """every chromosome of the features through one call, exactly the reference's tables -> (cells, votes) summed"""
    f = _features(features)
    cells, votes = R.state_aggregate(s, L, f, T, F, K, G)
    got_c, got_v = np.zeros_like(cells), np.zeros_like(votes)
    for chrom in np.unique(f[:, 0]):
        status, c, v = _call(gpu, s, L, int(chrom), f[f[:, 0] == chrom], T, F, K, G)
        assert status == 0, (what, T, F, K, G, int(chrom), status)
        got_c += c
        got_v += v
    assert np.array_equal(got_c, cells), (what, T, F, np.argwhere(got_c != cells)[:5].tolist())
    assert np.array_equal(got_v, votes), (what, T, F, np.argwhere(got_v != votes)[:5].tolist())
    assert np.all(got_v.sum(axis=-1) <= np.bincount(f[:, 5], minlength=G)[:, None, None])
    return got_c, got_v


# ---- 1: one diagonal region ----------------------------------------------------------------------------------------------------
ONE = _len_vec([(40, 40, 0, 0, 1, 1)])
ONE_FEATURES = [[1, 0, 1, 0, 1, 0, 0], [1, 39, 40, 39, 40, 1, 1], [1, 0, 3, 0, 3, 0, 1], [1, 37, 40, 37, 40, 1, 0], [1, 5, 13, 5, 13, 0, 0],
                [1, 0, 8, 0, 8, 1, 1], [1, 32, 40, 32, 40, 0, 0], [1, 10, 30, 10, 30, 1, 0], [1, 0, 20, 0, 20, 0, 1], [1, 20, 40, 20, 40, 1, 0],
                [1, 0, 37, 0, 37, 0, 0], [1, 3, 40, 3, 40, 1, 1], [1, 10, 30, 10, 30, 1, 0], [1, 2, 5, 17, 37, 0, 0], [1, 12, 20, 9, 10, 1, 1]]


@pytest.mark.parametrize("blocky", (False, True))
def test_one_diagonal_region(gpu, blocky):
    """lengths 1, 3, 8, 20 and 37 at T = 8, F = 4 (upsampling, identity, non-integer ratios), at both ends of the chromosome
    with flanks on negative bins and past the end, flipped and not, a duplicate, two interval pairs"""
    s = _state_vec(ONE, {1: _symmetric(40, 3, 11, blocky)})
    cells, votes = _check(gpu, s, ONE, ONE_FEATURES, 8, 4, 3, 2, "one region")
    given = np.bincount(_features(ONE_FEATURES)[:, 5])
    assert votes.any() and (votes.sum(axis=-1) < given[:, None, None]).any()      # some cells of some features lie wholly off the map


# ---- 2: seams -----------------------------------------------------------------------------------------------------------------
# chromosome 1: bins 0 - 29 and 35 - 64 (30 - 34 are uncovered) and the block between the two; chromosome 2: 20 bins
SEAMS = _len_vec([(30, 30, 0, 0, 1, 1), (30, 30, 0, 35, 0, 1), (30, 30, 35, 35, 1, 1), (20, 20, 0, 0, 1, 2)])
SEAM_FEATURES = [[1, 25, 40, 25, 40, 0, 0], [1, 28, 37, 28, 37, 0, 1], [1, 0, 65, 0, 65, 1, 0], [1, 30, 35, 30, 35, 0, 0],
                 [1, 10, 50, 10, 50, 1, 1], [1, 5, 15, 40, 60, 0, 0], [1, 25, 33, 33, 50, 1, 0], [1, 20, 45, 20, 45, 0, 0],
                 [2, 0, 20, 0, 20, 0, 0], [2, 5, 9, 5, 9, 1, 1], [2, 2, 6, 10, 19, 0, 0]]


def _seam_map():
    """K = 3.  Inside [20, 45)^2 the part of every region has ITS majority on state 0 or 1 (11 nodes of 20) and the rest on
    state 2, so that state 2 is the majority of the square as a whole and of no single region's part"""
    M = _symmetric(65, 3, 5)
    i, j = np.indices((65, 65))
    mostly = (3 * np.minimum(i, j) + 7 * np.maximum(i, j)) % 20 < 11
    lo, hi = (i >= 20) & (i < 30), (i >= 35) & (i < 45)
    lo_j, hi_j = (j >= 20) & (j < 30), (j >= 35) & (j < 45)
    M = np.where(lo & lo_j, np.where(mostly, 0, 2), M)
    M = np.where(hi & hi_j, np.where(mostly, 0, 2), M)
    M = np.where((lo & hi_j) | (hi & lo_j), np.where(mostly, 1, 2), M)
    return _state_vec(SEAMS, {1: M, 2: _symmetric(20, 3, 6)})


@pytest.mark.parametrize("T,F", ((4, 2), (1, 0), (1, 1), (7, 3)))
def test_seams(gpu, T, F):
    """features and interval pairs whose cells straddle both seams and the gap; at T = 1 the feature [20, 45) is one cell that
    takes the wave-per-cell path through all three regions"""
    _check(gpu, _seam_map(), SEAMS, SEAM_FEATURES, T, F, 3, 2, "seams")


def test_seam_vote_uses_the_total_over_all_regions(gpu):
    s = _seam_map()
    feature = [[1, 20, 45, 20, 45, 0, 0]]
    per_region = [R.state_aggregate(s, SEAMS[[r]], feature, 1, 0, 3, 1)[0][0, 0, 0] for r in range(3)]
    whole = R.state_aggregate(s, SEAMS, feature, 1, 0, 3, 1)[0][0, 0, 0]
    assert [int(np.argmax(h)) for h in per_region] == [0, 1, 0] and int(np.argmax(whole)) == 2 and np.array_equal(sum(per_region), whole)
    status, cells, votes = _call(gpu, s, SEAMS, 1, feature, 1, 0, 3, 1)
    assert status == 0 and cells[0, 0, 0].tolist() == whole.tolist() and votes[0, 0, 0].tolist() == [0, 0, 1]


# ---- 3: the wave-per-cell path and the counter width --------------------------------------------------------------------------
WIDE = _len_vec([(640, 640, 0, 0, 1, 1)])


@pytest.fixture(scope="module")
def wide_map():
    return _state_vec(WIDE, {1: _symmetric(640, 4, 21, blocky=True)})


def test_cells_above_two_to_the_sixteen(gpu):
    """T = 2 on 600 bins: 90,000 bin pairs a cell, about nine in ten of them in state 3, so one feature's counter of one cell
    passes 2^16"""
    M = _symmetric(640, 4, 22, blocky=True)
    rare = _symmetric(640, 10, 23) == 0
    s = _state_vec(WIDE, {1: np.where(rare, M, 3)})
    features = [[1, 20, 620, 20, 620, 0, 0], [1, 30, 630, 30, 630, 0, 1]]
    assert R.feature_hist(s, WIDE, features[0], 2, 0, 4).max() > 1 << 16
    cells, votes = _check(gpu, s, WIDE, features, 2, 0, 4, 1, "90,000 pairs a cell")
    assert cells.sum(axis=-1).max() == 2 * 90000 and votes.sum() == 2 * 4 and votes[..., 3].sum() == 2 * 4


def test_feature_of_600_bins_on_64_cells(gpu, wide_map):
    _check(gpu, wide_map, WIDE, [[1, 20, 620, 20, 620, 0, 0]], 64, 0, 4, 1, "600 bins at T = 64")


def test_both_sides_of_the_threshold(gpu, wide_map):
    """T = 2: features of 32 bins have cells of 16 x 16 = SMALL_AREA bin pairs (a lane per cell), of 33 and 34 bins cells of
    17 x 17 (a wave per cell); interval pairs of 30 x 34 bins (15 x 17 = 255) and of 32 x 34 (16 x 17 = 272); with flanks on
    negative bins and past the end in both paths"""
    assert aggregate.SMALL_AREA == 256
    assert aggregate.is_small(32, 32, 2) and not aggregate.is_small(33, 33, 2) and aggregate.is_small(30, 34, 2) and not aggregate.is_small(32, 34, 2)
    features = [[1, 100, 132, 100, 132, 0, 0], [1, 100, 133, 100, 133, 0, 0], [1, 300, 334, 300, 334, 0, 1], [1, 50, 80, 400, 434, 0, 0],
                [1, 50, 82, 400, 434, 0, 0], [1, 5, 45, 5, 45, 0, 0], [1, 600, 640, 600, 640, 0, 1], [1, 0, 32, 0, 32, 0, 0],
                [1, 608, 640, 608, 640, 0, 0]]
    _check(gpu, wide_map, WIDE, features, 2, 1, 4, 1, "threshold")


@pytest.mark.parametrize("k", (0, 1, 2, 3))
def test_wave_rows_at_every_byte_alignment(gpu, k):
    """a 1 x k off-diagonal region of another chromosome in front (none for k = 0) moves the slice of chromosome 1's 48 x 48
    diagonal region to byte k of the labels; the feature [4, 44) at T = 2, F = 1 has cells of 20 x 20 = 400 bin pairs, so it
    goes a wave per cell over rows of 20 bytes: a head, aligned words and a tail, split differently for every k"""
    L = _len_vec(([(1, k, 0, 0, 0, 2)] if k else []) + [(48, 48, 0, 0, 1, 1)])
    assert L[-1, 1] == k and not aggregate.is_small(40, 40, 2)
    s = _state_vec(L, {1: _symmetric(48, 5, 61, blocky=True), 2: _symmetric(4, 5, 62)})
    cells, votes = _check(gpu, s, L, [[1, 4, 44, 4, 44, 0, 0]], 2, 1, 5, 1, "the slice starts at byte %d" % k)
    assert cells[0, 1:3, 1:3].sum() == 40 * 40 and votes[0, 1:3, 1:3].sum() == 4


# ---- 4: ties ------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_state(gpu):
    i, j = np.indices((40, 40))
    s = _state_vec(ONE, {1: 1 + (i + j) % 2})                # states 1 and 2 interleaved, state 0 absent
    for T, features in ((4, [[1, 8, 24, 8, 24, 0, 0], [1, 0, 16, 20, 36, 0, 1]]), (1, [[1, 0, 40, 0, 40, 0, 0], [1, 0, 20, 20, 40, 0, 0]])):
        cells, votes = _check(gpu, s, ONE, features, T, 0, 3, 1, "ties")
        tied = (cells[0, ..., 1] == cells[0, ..., 2]) & (cells[0, ..., 1] > 0)
        assert tied.any() and np.all(votes[0, tied, 1] == len(features)) and np.all(votes[0, tied, 2] == 0)


# ---- 5: limits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 64))
def test_fewest_and_most_states(gpu, K):
    s = _state_vec(ONE, {1: _symmetric(40, K, 31)})
    _check(gpu, s, ONE, ONE_FEATURES, 8, 4, K, 2, "K")
    _check(gpu, s, ONE, [[1, 0, 40, 0, 40, 0, 0], [1, 2, 39, 2, 39, 1, 1]], 2, 0, K, 2, "K, a wave per cell")


def test_sixteen_groups_with_an_empty_one(gpu):
    s = _state_vec(ONE, {1: _symmetric(40, 3, 32)})
    groups = [g for g in range(16) if g != 7]
    features = [[1, 2 * g, 2 * g + 3 + g, 2 * g, 2 * g + 3 + g, g, g & 1] for g in groups] + [[1, 0, 40, 0, 40, 15, 0]]
    cells, votes = _check(gpu, s, ONE, features, 3, 1, 3, 16, "G = 16")
    assert not cells[7].any() and not votes[7].any() and cells[15].any()


def test_one_more_feature_than_a_chunk(gpu):
    s = _state_vec(ONE, {1: _symmetric(40, 3, 33)})
    rng = np.random.default_rng(34)
    a0 = rng.integers(0, 36, aggregate.CHUNK + 1)
    n = rng.integers(1, 5, aggregate.CHUNK + 1)
    features = [[1, x, x + m, x, x + m, 1, int(t & 1)] for t, (x, m) in enumerate(zip(a0, n))] + [[1, 3, 9, 3, 9, 0, 0]]
    cells, votes = _check(gpu, s, ONE, features, 3, 1, 3, 2, "CHUNK + 1")
    assert votes[1].sum(axis=-1).max() == aggregate.CHUNK + 1


@pytest.mark.parametrize("T,F", ((5, 3), (5, 4)))
def test_pile_that_is_no_multiple_of_a_tile(gpu, T, F):
    assert (T + 2 * F) ** 2 % aggregate.LANES
    s = _state_vec(ONE, {1: _symmetric(40, 3, 35)})
    _check(gpu, s, ONE, ONE_FEATURES, T, F, 3, 2, "P^2 = %d" % (T + 2 * F) ** 2)


def test_largest_pile(gpu):
    big = _len_vec([(64, 64, 0, 0, 1, 1)])
    s = _state_vec(big, {1: _symmetric(64, 2, 36, blocky=True)})
    cells, votes = _check(gpu, s, big, [[1, 20, 44, 20, 44, 0, 0], [1, 0, 64, 0, 64, 0, 1]], 64, 32, 2, 1, "P = 128")
    assert cells.shape == (1, 128, 128, 2)


# ---- 6: errors ----------------------------------------------------------------------------------------------------------------
def test_label_above_K(gpu):
    M = _symmetric(40, 3, 41)
    M[30:, 30:] = 5
    s = _state_vec(ONE, {1: M})
    inside, outside = _features([[1, 20, 32, 20, 32, 0, 0]]), _features([[1, 5, 15, 5, 15, 0, 0]])       # T = 4, F = 1: [17, 35) and [3, 18)
    for T, F in ((4, 1), (1, 0)):                            # a lane per cell
        with pytest.raises(RuntimeError):
            aggregate.state_aggregate(s, ONE, inside, T, F, K=3)
        status, cells, votes = _call(gpu, s, ONE, 1, inside, T, F, 3, 1)
        assert status == INVALID and _untouched(cells, votes), (T, F)
    got = aggregate.state_aggregate(s, ONE, outside, 4, 1, K=3)
    want = R.state_aggregate(s, ONE, outside, 4, 1, 3, 1)
    assert np.array_equal(got["cells"], want[0]) and np.array_equal(got["votes"], want[1])
    assert not aggregate.is_small(30, 30, 1)
    with pytest.raises(RuntimeError):                        # the same through the wave-per-cell path
        aggregate.state_aggregate(s, ONE, _features([[1, 5, 35, 5, 35, 0, 0]]), 1, 0, K=3)


def test_refusals(gpu):
    s = _state_vec(ONE, {1: _symmetric(40, 3, 42)})
    ok = [1, 5, 13, 5, 13, 0, 0]
    cases = (("flip = 2", [ok, [1, 5, 13, 5, 13, 0, 2]], 8, 4, 3, 1, INVALID), ("T = 65", [ok], 65, 0, 3, 1, UNSUPPORTED),
             ("a1 = a0", [ok, [1, 7, 7, 5, 13, 0, 0]], 8, 4, 3, 1, INVALID), ("b1 < b0", [[1, 5, 13, 9, 8, 0, 0]], 8, 4, 3, 1, INVALID),
             ("F = 33", [ok], 8, 33, 3, 1, UNSUPPORTED), ("T = 0", [ok], 0, 4, 3, 1, INVALID), ("F = -1", [ok], 8, -1, 3, 1, INVALID),
             ("G = 17", [ok], 8, 4, 3, 17, UNSUPPORTED), ("K = 65", [ok], 8, 4, 65, 1, UNSUPPORTED),
             ("a coordinate of 2^30", [[1, 5, 1 << 30, 5, 13, 0, 0]], 8, 4, 3, 1, UNSUPPORTED))
    for what, features, T, F, K, G, code in cases:
        status, cells, votes = _call(gpu, s, ONE, 1, features, T, F, K, G, small=T > 64 or T < 1 or F > 32 or F < 0 or G > 16 or K > 64)
        assert status == code and _untouched(cells, votes), (what, status)
    # G P P K <= 2^24 follows from G <= 16, P <= 128 and K <= 64: the largest table any call can ask for is exactly at the limit
    assert aggregate.MAX_GROUPS * (aggregate.MAX_BODY + 2 * aggregate.MAX_FLANK) ** 2 * 64 == aggregate.MAX_TABLE == 1 << 24
    bad = ONE.copy()
    bad[0, 1] = 1                                            # the region's nodes would end past the labels
    bad[0, 2] = bad[0, 1] + bad[0, 0]
    status, cells, votes = _call(gpu, s, bad, 1, [ok], 8, 4, 3, 1)
    assert status == INVALID and _untouched(cells, votes)
    status, cells, votes = _call(gpu, s, np.concatenate([ONE] * 65), 1, [ok], 8, 4, 3, 1)
    assert status == UNSUPPORTED and _untouched(cells, votes)


def test_no_features_and_no_flips(gpu):
    s = _state_vec(ONE, {1: _symmetric(40, 3, 43)})
    status, cells, votes = _call(gpu, s, ONE, 1, np.zeros((0, 7), dtype=np.int64), 8, 4, 3, 2)
    assert status == 0 and not cells.any() and not votes.any()
    unflipped = [f[:6] + [0] for f in ONE_FEATURES]
    status, cells, votes = _call(gpu, s, ONE, 1, unflipped, 8, 4, 3, 2, flip=None)
    want = R.state_aggregate(s, ONE, unflipped, 8, 4, 3, 2)
    assert status == 0 and np.array_equal(cells, want[0]) and np.array_equal(votes, want[1])


def test_two_runs_give_the_same_bytes_and_the_chromosomes_are_summed(gpu):
    s = _seam_map()
    a = aggregate.state_aggregate(s, SEAMS, SEAM_FEATURES, 4, 2)
    b = aggregate.state_aggregate(s, SEAMS, SEAM_FEATURES, 4, 2)
    want = R.state_aggregate(s, SEAMS, SEAM_FEATURES, 4, 2, 3, 2)
    assert a["cells"].tobytes() == b["cells"].tobytes() and a["votes"].tobytes() == b["votes"].tobytes()
    assert np.array_equal(a["cells"], want[0]) and np.array_equal(a["votes"], want[1])
    assert a["n_features"].tolist() == [7, 4] and a["features_chrom"].tolist() == [[1, 8], [2, 3]]
    assert (int(a["K"]), int(a["G"]), int(a["body"]), int(a["flank"])) == (3, 2, 4, 2)


# ---- 7, 8: against the existing kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,F", ((5, 2), (1, 3), (9, 0)))
def test_identity_with_the_pileup_kernel(gpu, T, F):
    """T odd, n = T, no flip: every pile cell is one bin pair, so cells == votes == the pile of --pileup around the centre
    a0 + (T - 1) / 2 with w = F + (T - 1) / 2"""
    s = _seam_map()
    h = (T - 1) // 2
    starts = {1: (0, 3, 24, 27, 31, 33, 40, 60), 2: (0, 7, 15)}
    features = [[c, a, a + T, a, a + T, t & 1, 0] for c in starts for t, a in enumerate(starts[c])] + [[1, 10, 10 + T, 38, 38 + T, 0, 0]]
    centres = [[f[0], f[1] + h, f[3] + h, f[5], 0] for f in features]
    got = aggregate.state_aggregate(s, SEAMS, features, T, F, K=3, G=2)
    pile = pileup.state_pileup(s, SEAMS, np.array(centres, dtype=np.int64), F + h, K=3, G=2)["obs"]
    assert np.array_equal(got["cells"], pile) and np.array_equal(got["votes"], pile) and pile.any()


def test_counts_against_the_rectangle_query(gpu):
    """A = B and n >= T: the body cells tile A x A, so their `cells` sum to 2 (the query's counts) - (the diagonal nodes in A)"""
    s = _seam_map()
    T, F = 4, 2
    features = [f for f in SEAM_FEATURES if f[1] == f[3] and f[2] == f[4] and f[2] - f[1] >= T]
    assert len(features) >= 6
    counts = query.state_query(s, SEAMS, np.array([f[:5] for f in features], dtype=np.int64), K=3)["counts"]
    for f, inside in zip(features, counts):
        singles = np.array([[f[0], p, p + 1, p, p + 1] for p in range(f[1], f[2])], dtype=np.int64)
        on_diagonal = query.state_query(s, SEAMS, singles, K=3)["counts"].sum(axis=0)
        got = aggregate.state_aggregate(s, SEAMS, [f[:5] + [0, f[6]]], T, F, K=3, G=1)["cells"][0]
        assert np.array_equal(got[F:F + T, F:F + T].sum(axis=(0, 1)), 2 * inside - on_diagonal), f


# ---- 9: the command line's files ----------------------------------------------------------------------------------------------
def test_aggregate_files_round_trip(tmp_path):
    import scipy.io
    L = _len_vec([(48, 48, 0, 0, 1, 1)])
    s = _state_vec(L, {1: _symmetric(48, 4, 51, blocky=True)})
    path = os.path.join(str(tmp_path), "estimate_ou_7.mat")
    scipy.io.savemat(path, dict(state_vec=s.reshape(1, -1), state_vec_smooth=(3 - s).reshape(1, -1), len_vec=L))
    bed = os.path.join(str(tmp_path), "tads.bed")
    with open(bed, "w") as fh:
        fh.write("#chrom start stop name score strand\nchr1 500000 1000000 tad 0 +\nchr1 1200000 2050000 tad 0 -\n"
                 "chr1 100000 140000 tad\nchr1 300000 1700000 domain\nchrX 0 5 tad\nchr1 1000000 1150000\n")
    out = aggregate.aggregate_files(path, str(tmp_path / "out"), 50000, field="state_vec_smooth", bed=bed, body=4, flank=2,
                                    shift_bp=250000, min_bp=50000)
    assert os.path.basename(out) == "aggregate_estimate_ou_7.npz"
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["aggregate_estimate_ou_7.npz", "aggregate_estimate_ou_7.txt",
                                                         "aggregate_estimate_ou_7_domain.png", "aggregate_estimate_ou_7_feature.png",
                                                         "aggregate_estimate_ou_7_tad.png"]
    z = np.load(out, allow_pickle=False)
    for key in ("cells", "votes", "ctl_cells", "ctl_votes", "log2_ratio", "n_features", "names", "skipped_lines", "skipped_short", "body",
                "flank", "shift", "K", "len_vec", "palette", "resolution", "aggregate_field", "features_file", "feature_kind", "shift_bp",
                "min_bp", "features_chrom"):
        assert key in z.files, key
    read = aggregate.read_features(bed, L, 50000, 50000)
    assert read["names"] == ["tad", "domain", "feature"] and read["skipped_lines"] == 1 and read["skipped_short"] == 1
    assert read["features"].tolist() == [[1, 10, 20, 10, 20, 0, 0], [1, 24, 41, 24, 41, 0, 1], [1, 6, 34, 6, 34, 1, 0], [1, 20, 23, 20, 23, 2, 0]]
    want = R.state_aggregate(3 - s, L, aggregate.with_controls(read["features"], 5, 3), 4, 2, 4, 6)
    assert np.array_equal(z["cells"], want[0][:3]) and np.array_equal(z["votes"], want[1][:3]) and z["votes"].any()
    assert np.array_equal(z["ctl_cells"], want[0][3:]) and np.array_equal(z["ctl_votes"], want[1][3:]) and z["ctl_votes"].any()
    assert np.array_equal(z["log2_ratio"], pileup.log2_ratio(want[1][:3], want[1][3:]), equal_nan=True)
    assert (int(z["body"]), int(z["flank"]), int(z["shift"]), int(z["K"]), int(z["skipped_lines"]), int(z["skipped_short"])) == (4, 2, 5, 4, 1, 1)
    assert z["names"].tolist() == read["names"] and np.array_equal(z["len_vec"], L) and str(z["aggregate_field"]) == "state_vec_smooth"
    lines = open(os.path.join(str(tmp_path / "out"), "aggregate_estimate_ou_7.txt")).read().splitlines()
    assert lines[0].startswith("#name\tu\tv\tu_pos\tv_pos\tfeatures\t") and len(lines) == 1 + 3 * 8 * 8
    for ln in lines[1:]:
        c = ln.split("\t")
        g, u, v = read["names"].index(c[0]), int(c[1]), int(c[2])
        assert len(c) == 12 + 4 and [int(x) for x in c[12:]] == want[1][g, u, v].tolist() and int(c[9]) == want[0][g, u, v].sum()
    from phylo_hmrf_amd.render import PNG_SIGNATURE
    png = open(os.path.join(str(tmp_path / "out"), "aggregate_estimate_ou_7_tad.png"), "rb").read()
    assert png.startswith(PNG_SIGNATURE) and png[16:24] == (64).to_bytes(4, "big") * 2            # 8 cells of 8 pixels a side
