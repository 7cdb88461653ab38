"""CPU: the post-processing's smoothing rule (tests/smooth_reference.py, the yardstick of the GPU pass) on hand-built maps
with hand-derived answers, the facts that let the device work on a diagonal block's upper triangle alone, the state-file
writer byte for byte, input validation ahead of any library call, and the command line's new options."""
import os

import numpy as np
import pytest
from scipy import ndimage

from tests import smooth_reference as S


def _upper(M):
    return S.upper_nodes(np.asarray(M), True)


def _smooth_full(M, diagonal, **kw):
    M = np.asarray(M)
    H, W = M.shape
    out = S.smooth_region(S.upper_nodes(M, diagonal), H, W, diagonal, **kw)
    return S.full_matrix(out, H, W, diagonal)


# ---- the rule on hand-built maps -------------------------------------------------------------------------------------
def test_island_off_the_diagonal_and_its_mirror():
    M = np.zeros((12, 12), dtype=np.int64)
    M[2:4, 7:9] = 1                      # 2 x 2 island, j - i >= 4: its mirror at rows 7-8, columns 2-3 is another component
    M[7:9, 2:4] = 1
    out, n_small, n_changed = S.smooth_pass(M, 3, 4)
    assert (n_small, n_changed) == (2, 2)          # both islands; the background (area 136) is large
    assert not out.any()
    # one pixel more than the threshold: both stay
    out, n_small, n_changed = S.smooth_pass(M, 3, 3)
    assert (n_small, n_changed) == (0, 0) and np.array_equal(out, M)
    # the same through the upper triangle's node order
    assert not _smooth_full(M, True, window=3, max_area=4).any()


def test_self_mirror_island_area_exactly_a_and_a_plus_one():
    M = np.zeros((10, 10), dtype=np.int64)
    M[4:6, 4:6] = 1                      # stored nodes (4,4) (4,5) (5,5): full-matrix area 2 * 3 - 2 = 4
    assert int((_upper(M) == 1).sum()) == 3
    assert not _smooth_full(M, True, window=3, max_area=4).any()                        # area == A: small
    assert np.array_equal(_smooth_full(M, True, window=3, max_area=3), M)               # area == A + 1: kept


def _fifty_fifty_map():
    M = np.array([[0, 0, 0, 1, 1],
                  [0, 0, 0, 1, 1],
                  [0, 0, 2, 1, 1],
                  [0, 0, 1, 1, 1],
                  [0, 0, 1, 1, 1]], dtype=np.int64)
    return M


def test_a_fifty_fifty_vote_keeps_the_component():
    M = _fifty_fifty_map()               # the island's 8 neighbours: four 0, four 1 -> 4 > 0.5 * 8 fails
    out, n_small, n_changed = S.smooth_pass(M, 3, 1)
    assert (n_small, n_changed) == (1, 0) and np.array_equal(out, M)
    M[3, 2] = 0                          # five 0, three 1: 0 wins
    out, n_small, n_changed = S.smooth_pass(M, 3, 1)
    want = M.copy()
    want[2, 2] = 0
    assert (n_small, n_changed) == (1, 1) and np.array_equal(out, want)


def test_an_island_whose_windows_all_cross_the_border_keeps_its_state():
    M = np.zeros((4, 4), dtype=np.int64)
    M[1, 1] = 1
    assert np.array_equal(_smooth_full(M, False, window=5, max_area=10), M)   # h = 2: no pixel of a 4 x 4 map votes
    assert not _smooth_full(M, False, window=3, max_area=10).any()            # h = 1: (1, 1) votes
    M = np.zeros((4, 4), dtype=np.int64)
    M[0, 0] = 1
    assert np.array_equal(_smooth_full(M, False, window=3, max_area=10), M)   # a corner pixel never votes


def test_two_adjacent_small_components_decide_on_the_same_map():
    M = np.zeros((6, 6), dtype=np.int64)
    M[2, 2] = 1                          # A: neighbours four 0 and four 2 (B) -> tie, keeps 1
    M[1, 3] = M[2, 3] = M[3, 3] = M[3, 2] = 2   # B (area 4): 20 votes for 0, 4 for 1 -> becomes 0
    out, n_small, n_changed = S.smooth_pass(M, 3, 4)
    want = np.zeros_like(M)
    want[2, 2] = 1
    assert (n_small, n_changed) == (2, 1) and np.array_equal(out, want)
    # the second pass sees B's new state: A now has eight 0 around it
    assert not _smooth_full(M, False, window=3, max_area=4, n_iter=2).any()


def test_an_h_by_w_block_uses_each_nodes_row_and_column():
    M = np.zeros((4, 7), dtype=np.int64)
    M[2:, :] = 2
    M[1, 5] = 1                          # window: five 0, three 2 -> 0
    M[2, 1] = 1                          # window: three 0, five 2 -> 2
    want = M.copy()
    want[1, 5], want[2, 1] = 0, 2
    assert np.array_equal(_smooth_full(M, False, window=3, max_area=1), want)
    # node order: row-major H x W
    out = S.smooth_region(M.reshape(-1), 4, 7, False, window=3, max_area=1)
    assert np.array_equal(out, want.reshape(-1))


def test_an_even_window_reaches_window_over_two_bins_each_way():
    M = np.zeros((7, 7), dtype=np.int64)
    M[1:6, 1:6] = 2
    M[2:5, 2:5] = 0
    M[3, 3] = 1                          # 5 x 5 window: sixteen 2 (the ring at distance 2), eight 0
    want = M.copy()
    want[3, 3] = 2
    assert np.array_equal(_smooth_full(M, False, window=4, max_area=1), want)       # h = 4 // 2 = 2
    want[3, 3] = 0
    assert np.array_equal(_smooth_full(M, False, window=3, max_area=1), want)       # h = 1


def test_default_area_follows_the_region_height():
    assert S.default_max_area(99) == 25 and S.default_max_area(100) == 80
    from phylo_hmrf_amd.smooth import default_max_area
    assert default_max_area(99) == 25 and default_max_area(100) == 80


# ---- the upper-triangle facts the device relies on -------------------------------------------------------------------
def _noisy_symmetric(rng, n, K, p=0.3):
    from phylo_hmrf_amd import synthetic
    img = synthetic.label_image(rng, n, n, K, mean_run=6)
    noise = rng.random((n, n)) < p
    img[noise] = rng.integers(0, K, int(noise.sum()))
    return S.full_matrix(S.upper_nodes(img, True), n, n, True)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_upper_triangle_components_are_the_full_matrix_components(seed):
    rng = np.random.default_rng(seed)
    n, K = 40, 4
    M = _noisy_symmetric(rng, n, K)
    iu = np.triu_indices(n)
    upper_mask = np.zeros((n, n), dtype=bool)
    upper_mask[iu] = True
    st = np.ones((3, 3), dtype=bool)
    for s in range(K):
        full, _ = ndimage.label(M == s, structure=st)
        up, _ = ndimage.label((M == s) & upper_mask, structure=st)
        a, b = full[iu], up[iu]
        sel = a > 0
        # the same partition of the upper nodes
        pairs = np.unique(np.stack([a[sel], b[sel]]), axis=1)
        assert len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))
        for c in np.unique(b[sel]):
            nodes = b == c
            comp = a[nodes][0]
            area_full = int((full == comp).sum())
            i, j = iu[0][nodes], iu[1][nodes]
            self_mirror = bool(np.any(j - i <= 1))
            # self-mirror exactly when the component holds a node with j - i <= 1 ...
            mirror_comp = full[j[0], i[0]]
            assert self_mirror == (mirror_comp == comp)
            # ... with area 2 * nodes - diagonal nodes; otherwise its twin is separate and as large
            if self_mirror:
                assert area_full == 2 * int(nodes.sum()) - int((i == j).sum())
            else:
                assert area_full == int(nodes.sum()) == int((full == mirror_comp).sum())


def test_smoothing_a_symmetric_map_keeps_it_symmetric():
    rng = np.random.default_rng(5)
    M = _noisy_symmetric(rng, 50, 6)
    out, n_small, n_changed = S.smooth_pass(M, 5, 25)
    assert n_changed > 0 and np.array_equal(out, out.T)


# ---- the writer ------------------------------------------------------------------------------------------------------
LEN_VEC = np.array([[6, 0, 6, 3, 3, 10, 10, 0, 1, 22],        # chr22: 3-bin diagonal block from bin 10
                    [6, 6, 12, 2, 3, 10, 20, 1, 0, 22],       # chr22: 2 x 3 off-diagonal block, rows from bin 10, columns from 20
                    [1, 12, 13, 1, 1, 4, 4, 0, 1, 21]])       # chr21: one bin


def test_writer_byte_for_byte(tmp_path):
    from phylo_hmrf_amd.smooth import write_state_files
    state_vec = np.arange(13, dtype=np.int64).reshape(1, 13)        # as a .mat file holds it
    files = write_state_files(state_vec, LEN_VEC, 50000, str(tmp_path), "ori")
    assert sorted(os.path.basename(f) for f in files) == ["estimate_test21.ori.txt", "estimate_test22.ori.txt",
                                                          "test21.region.txt", "test22.region.txt"]
    want22 = ("22\t500000\t550000\t22\t500000\t550000\t1\r\n"       # (0, 0)
              "22\t500000\t550000\t22\t550000\t600000\t2\r\n"       # (0, 1)
              "22\t500000\t550000\t22\t600000\t650000\t3\r\n"       # (0, 2)
              "22\t550000\t600000\t22\t550000\t600000\t4\r\n"       # (1, 1)
              "22\t550000\t600000\t22\t600000\t650000\t5\r\n"       # (1, 2)
              "22\t600000\t650000\t22\t600000\t650000\t6\r\n"       # (2, 2)
              "22\t500000\t550000\t22\t1000000\t1050000\t7\r\n"     # off-diagonal (0, 0)
              "22\t500000\t550000\t22\t1050000\t1100000\t8\r\n"
              "22\t500000\t550000\t22\t1100000\t1150000\t9\r\n"
              "22\t550000\t600000\t22\t1000000\t1050000\t10\r\n"    # (1, 0)
              "22\t550000\t600000\t22\t1050000\t1100000\t11\r\n"
              "22\t550000\t600000\t22\t1100000\t1150000\t12\r\n")
    assert (tmp_path / "estimate_test22.ori.txt").read_bytes() == want22.encode()
    assert (tmp_path / "estimate_test21.ori.txt").read_bytes() == b"21\t200000\t250000\t21\t200000\t250000\t13\r\n"
    assert (tmp_path / "test22.region.txt").read_bytes() == b"6\t1\t6\t3\t3\t10\t10\n6\t7\t12\t2\t3\t10\t20\n"
    assert (tmp_path / "test21.region.txt").read_bytes() == b"1\t1\t1\t1\t1\t4\t4\n"


def test_writer_in_chunks_matches_one_chunk(tmp_path):
    from phylo_hmrf_amd import smooth
    rng = np.random.default_rng(0)
    lv = np.array([[55, 0, 55, 10, 10, 3, 3, 0, 1, 7], [21, 55, 76, 3, 7, 3, 20, 1, 0, 7]])
    sv = rng.integers(0, 64, 76)
    for chunk, d in ((1 << 21, "a"), (4, "b")):
        with open(str(tmp_path / d), "wb") as fh:
            for row in lv:
                smooth._region_lines(fh, 7, 1000, row, sv[row[1]:row[2]], chunk=chunk)
    a = (tmp_path / "a").read_bytes()
    assert a == (tmp_path / "b").read_bytes()
    lines = a.split(b"\r\n")[:-1]
    assert len(lines) == 76
    iu = np.triu_indices(10)
    for v in (0, 9, 10, 54):
        f = [int(x) for x in lines[v].split(b"\t")]
        assert f == [7, (3 + iu[0][v]) * 1000, (4 + iu[0][v]) * 1000, 7, (3 + iu[1][v]) * 1000, (4 + iu[1][v]) * 1000, sv[v] + 1]


# ---- validation before the library -----------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from phylo_hmrf_amd import _lib

    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "require_gpu", refuse)


GOOD_SV = np.zeros(13, dtype=np.int64)


@pytest.mark.parametrize("sv", [np.full(13, -1), np.full(13, 64), np.full(13, 1.5), np.full(13, np.nan),
                                np.array(["a"] * 13)])
def test_invalid_state_vec_is_refused_before_the_library(no_library, sv, tmp_path):
    from phylo_hmrf_amd.smooth import smooth_states, write_state_files
    with pytest.raises(ValueError):
        smooth_states(sv, LEN_VEC)
    with pytest.raises(ValueError):
        write_state_files(sv, LEN_VEC, 50000, str(tmp_path), "ori")


def _bad_len_vecs():
    out = [LEN_VEC[:, :9]]                                   # too few columns
    lv = LEN_VEC.copy(); lv[0, 2] = 5; out.append(lv)        # slice too short for the block
    lv = LEN_VEC.copy(); lv[1, 4] = 4; out.append(lv)        # 2 x 4 does not hold 6 nodes
    lv = LEN_VEC.copy(); lv[0, 4] = 4; out.append(lv)        # non-square diagonal block
    lv = LEN_VEC.copy(); lv[2, 2] = 14; lv[2, 0] = 2; out.append(lv)   # beyond state_vec
    lv = LEN_VEC.copy(); lv[1, 8] = 2; out.append(lv)        # type neither 0 nor 1
    out.append(LEN_VEC + 0.5)                                # not integral
    return out


@pytest.mark.parametrize("k", range(7))
def test_invalid_len_vec_is_refused_before_the_library(no_library, k, tmp_path):
    from phylo_hmrf_amd.smooth import smooth_states, write_state_files
    lv = _bad_len_vecs()[k]
    with pytest.raises(ValueError):
        smooth_states(GOOD_SV, lv)
    with pytest.raises(ValueError):
        write_state_files(GOOD_SV, lv, 50000, str(tmp_path), "ori")


def test_invalid_settings_are_refused_before_the_library(no_library):
    from phylo_hmrf_amd.smooth import smooth_states
    for kw in (dict(window=0), dict(n_iter=-1), dict(max_area=-2)):
        with pytest.raises(ValueError):
            smooth_states(GOOD_SV, LEN_VEC, **kw)


# ---- command line ----------------------------------------------------------------------------------------------------
def test_command_line_options_and_defaults():
    import phylo_hmrf as cli
    o = cli.parse_args([])
    assert (o.postprocess, o.smooth_window, o.smooth_area, o.smooth_iter) == ("", "5", "-1", "1")
    assert o.threshold == "0.001"                            # the EM threshold is a different option
    o = cli.parse_args(["--postprocess", "x.mat", "--smooth_window", "7", "--smooth_area", "30", "--smooth_iter", "2"])
    assert (o.postprocess, o.smooth_window, o.smooth_area, o.smooth_iter) == ("x.mat", "7", "30", "2")


def test_command_line_postprocess_refuses_a_file_without_states(no_library, tmp_path):
    import scipy.io
    import phylo_hmrf as cli
    p = str(tmp_path / "x.mat")
    scipy.io.savemat(p, {"len_vec": LEN_VEC})
    with pytest.raises(ValueError):
        cli.run("4", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", str(tmp_path),
                postprocess=p)
