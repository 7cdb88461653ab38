"""No GPU: the definition of the genome tracks (tests/tracks_reference.py) on hand-worked cases, and the host side of
phylo_hmrf_amd.tracks: the chromosome merge, the per-bin summary, the windows, the text lines and the command line's checks."""
import math
import os

import numpy as np
import pytest

from phylo_hmrf_amd import tracks
from tests import tracks_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a 3 x 3 diagonal block, stored (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); its full matrix:
#   0 1 1
#   1 0 2
#   1 2 1
DIAG = [0, 1, 1, 0, 2, 1]
# a 2 x 3 off-diagonal block with dist0 = 4; its matrix and the distances |4 + j - i| of its cells:
#   0 1 2      4 5 6
#   2 2 0      3 4 5
OFF = [0, 1, 2, 2, 2, 0]


def _same(got, rows, cols=None):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64
    assert got[0].tolist() == rows
    assert got[1].tolist() == (rows if cols is None else cols)


# ---- the definition, by hand ------------------------------------------------------------------------------------------------
def test_diagonal_block_by_hand():
    _same(R.tracks(DIAG, 3, 3, True, 0, 3, 0, -1), [[1, 2, 0], [1, 1, 1], [0, 2, 1]])
    _same(R.tracks(DIAG, 3, 3, True, 0, 3, 0, 0), [[1, 0, 0], [1, 0, 0], [0, 1, 0]])
    _same(R.tracks(DIAG, 3, 3, True, 0, 3, 1, 1), [[0, 1, 0], [0, 1, 1], [0, 0, 1]])
    _same(R.tracks(DIAG, 3, 3, True, 0, 3, 3, -1), [[0, 0, 0]] * 3)


def test_off_diagonal_block_by_hand():
    _same(R.tracks(OFF, 2, 3, False, 4, 3, 0, -1), [[1, 1, 1], [1, 0, 2]], [[1, 0, 1], [0, 1, 1], [1, 0, 1]])
    _same(R.tracks(OFF, 2, 3, False, 4, 3, 4, 5), [[1, 1, 0], [1, 0, 1]], [[1, 0, 0], [0, 1, 1], [1, 0, 0]])
    _same(R.tracks(OFF, 2, 3, False, 4, 3, 0, 3), [[0, 0, 0], [0, 0, 1]], [[0, 0, 1], [0, 0, 0], [0, 0, 0]])
    _same(R.tracks(OFF, 2, 3, False, 4, 3, 7, 9), [[0, 0, 0]] * 2, [[0, 0, 0]] * 3)


def test_one_window_cuts_through_both_blocks():
    """(1, 4): the diagonal block loses its diagonal, the off-diagonal block its cells at distances 5 and 6"""
    _same(R.tracks(DIAG, 3, 3, True, 0, 3, 1, 4), [[0, 2, 0], [0, 1, 1], [0, 1, 1]])
    _same(R.tracks(OFF, 2, 3, False, 4, 3, 1, 4), [[1, 0, 0], [0, 0, 2]], [[1, 0, 1], [0, 0, 1], [0, 0, 0]])


def test_a_state_outside_the_window_is_not_looked_at():
    bad = list(OFF)
    bad[2] = 9                                               # cell (0, 2) at distance 6
    _same(R.tracks(bad, 2, 3, False, 4, 3, 0, 5), [[1, 1, 0], [1, 0, 2]], [[1, 0, 1], [0, 1, 1], [1, 0, 0]])
    with pytest.raises(AssertionError):
        R.tracks(bad, 2, 3, False, 4, 3, 0, -1)


@pytest.mark.parametrize("H,W,diag,dist0", [(7, 7, True, 0), (1, 1, True, 0), (5, 9, False, 0), (9, 5, False, -3), (4, 6, False, 40)])
def test_sums_under_the_unlimited_window(H, W, diag, dist0):
    rng = np.random.default_rng(H * 31 + W)
    n = H * (H + 1) // 2 if diag else H * W
    labels = rng.integers(0, 4, n)
    rows, cols = R.tracks(labels, H, W, diag, dist0, 4, 0, -1)
    if diag:
        assert rows.sum() == H * H == 2 * n - H and np.array_equal(rows, cols)
    else:
        assert rows.sum() == n and cols.sum() == n
        assert np.array_equal(rows.sum(axis=0), cols.sum(axis=0))
        assert np.array_equal(rows.sum(axis=0), np.bincount(labels, minlength=4))
    assert np.all(rows.sum(axis=1) == W) and np.all(cols.sum(axis=1) == H)
    # every distance lies in exactly one of three windows
    parts = [R.tracks(labels, H, W, diag, dist0, 4, lo, hi) for lo, hi in ((0, 1), (2, 5), (6, -1))]
    assert np.array_equal(sum(p[0] for p in parts), rows) and np.array_equal(sum(p[1] for p in parts), cols)


# ---- the chromosome merge ---------------------------------------------------------------------------------------------------
def _chromosome():
    """chromosome 3: diagonal regions on bins 0 - 2 and 5 - 6 and the off-diagonal region between them; bins 3, 4 uncovered"""
    rng = np.random.default_rng(5)
    a, b, c = rng.integers(0, 3, 6), rng.integers(0, 3, 3), rng.integers(0, 3, 6)
    s = np.concatenate([a, c, b])
    L = np.array([[6, 0, 6, 3, 3, 0, 0, 0, 1, 3],
                  [6, 6, 12, 3, 2, 0, 5, 1, 0, 3],
                  [3, 12, 15, 2, 2, 5, 5, 2, 1, 3]], dtype=np.int64)
    G = np.full((7, 7), -1, dtype=np.int64)                  # the chromosome-wide matrix, assembled by hand
    G[0:3, 0:3] = R.full(a, 3, 3, True)
    G[5:7, 5:7] = R.full(b, 2, 2, True)
    G[0:3, 5:7] = c.reshape(3, 2)
    G[5:7, 0:3] = c.reshape(3, 2).T
    return s, L, G


def test_merged_track_is_the_row_composition_of_the_chromosome_wide_matrix():
    s, L, G = _chromosome()
    want = np.stack([np.bincount(row[row >= 0], minlength=3) for row in G])
    assert want[3].sum() == 0 and want[4].sum() == 0 and want.sum() == 9 + 4 + 2 * 6
    ref = R.state_tracks(s, L, [(0, -1), (1, 5)], 3)
    assert ref["chrom"].tolist() == [3]
    assert np.array_equal(ref["track_3"][0], want)
    rows = [ref["rows_%d" % r] for r in range(3)]
    cols = [None, ref["cols_1"], None]
    got = tracks.merge_tracks(rows, cols, L, 3)
    assert got.dtype == np.int64 and got.shape == (2, 7, 3)
    assert np.array_equal(got[0], want)
    assert np.array_equal(got, ref["track_3"])
    # the window (1, 5) on the chromosome-wide matrix
    ii, jj = np.indices(G.shape)
    d = np.abs(jj - ii)
    cut = np.where((d >= 1) & (d <= 5), G, -1)
    assert np.array_equal(got[1], np.stack([np.bincount(row[row >= 0], minlength=3) for row in cut]))
    assert tracks.covered_bins(L, 3).tolist() == [True, True, True, False, False, True, True]
    assert tracks.chromosomes(L).tolist() == [3]


def test_merge_keeps_chromosomes_apart():
    s, L, _ = _chromosome()
    L2 = np.concatenate([L, [[3, 15, 18, 2, 2, 1, 1, 3, 1, 7]]]).astype(np.int64)
    s2 = np.concatenate([s, [2, 2, 2]])
    ref = R.state_tracks(s2, L2, [(0, -1)], 3)
    assert ref["chrom"].tolist() == [3, 7] and tracks.chromosomes(L2).tolist() == [3, 7]
    assert np.array_equal(ref["track_3"], R.state_tracks(s, L, [(0, -1)], 3)["track_3"])
    assert ref["track_7"][0].tolist() == [[0, 0, 0], [0, 0, 2], [0, 0, 2]]
    rows = [ref["rows_%d" % r] for r in range(4)]
    got = tracks.merge_tracks(rows, [None, ref["cols_1"], None, None], L2, 7)
    assert np.array_equal(got, ref["track_7"])


# ---- the summary ------------------------------------------------------------------------------------------------------------
def test_summary_ties_empty_bins_and_switch():
    t = np.array([[2, 2, 0],        # a tie: the lowest state
                  [2, 2, 0],        # equal to the bin before: switch 0
                  [0, 0, 5],        # shares no state with the bin before: switch 1
                  [0, 0, 0],        # empty
                  [1, 0, 3],        # after an empty bin: no switch
                  [0, 3, 3]], dtype=np.int64)
    sm = tracks.track_summary(t)
    assert sm["total"].dtype == np.float64 and sm["total"].tolist() == [4, 4, 5, 0, 4, 6]
    assert sm["dominant"].dtype == np.int64 and sm["dominant"].tolist() == [0, 0, 2, -1, 2, 1]
    assert sm["share"][[0, 1, 2, 4, 5]].tolist() == [0.5, 0.5, 1.0, 0.75, 0.5] and math.isnan(sm["share"][3])
    assert sm["entropy"][[0, 1, 2, 5]].tolist() == [1.0, 1.0, 0.0, 1.0] and math.isnan(sm["entropy"][3])
    assert sm["entropy"][4] == pytest.approx(-(0.25 * math.log2(0.25) + 0.75 * math.log2(0.75)), abs=1e-15)
    assert math.isnan(sm["switch"][0]) and math.isnan(sm["switch"][3]) and math.isnan(sm["switch"][4])
    assert sm["switch"][[1, 2]].tolist() == [0.0, 1.0]
    assert sm["switch"][5] == pytest.approx(0.5 * (0.25 + 0.5 + 0.25), abs=1e-15)


def test_summary_against_the_restatement():
    rng = np.random.default_rng(11)
    t = rng.integers(0, 50, (40, 6)) * (rng.random((40, 1)) < 0.8)
    sm, ref = tracks.track_summary(t.astype(np.int64)), R.summary(t)
    assert sm["dominant"].tolist() == ref["dominant"] and sm["total"].tolist() == ref["total"]
    for name in ("share", "entropy", "switch"):
        np.testing.assert_allclose(sm[name], np.array(ref[name]), rtol=0, atol=1e-12, equal_nan=True)
    empty = tracks.track_summary(np.zeros((0, 3), dtype=np.int64))
    assert all(empty[k].shape == (0,) for k in ("total", "dominant", "share", "entropy", "switch"))
    one = tracks.track_summary(np.array([[0, 4]]))
    assert one["dominant"].tolist() == [1] and math.isnan(one["switch"][0])
    with pytest.raises(ValueError):
        tracks.track_summary(np.zeros((2, 3, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        tracks.track_summary(np.zeros((2, 3)))


# ---- windows ----------------------------------------------------------------------------------------------------------------
def test_windows_from_bp_to_bins():
    assert tracks.parse_windows("0-", 10000) == [(0, -1)]
    assert tracks.parse_windows("0-2000000", 10000) == [(0, 200)]
    assert tracks.parse_windows("15000-25000", 10000) == [(2, 2)]          # ceil(1.5), floor(2.5)
    assert tracks.parse_windows("10000-10000", 10000) == [(1, 1)]
    assert tracks.parse_windows("1-", 50000) == [(1, -1)]
    assert tracks.parse_windows("0-0, 50000-99999 ,100000-", 50000) == [(0, 0), (1, 1), (2, -1)]
    assert len(tracks.parse_windows(",".join(["0-"] * tracks.MAX_WINDOWS), 1)) == tracks.MAX_WINDOWS == 8


@pytest.mark.parametrize("text,res", [
    ("15000-19000", 10000),          # holds no multiple of the resolution
    ("1-9999", 10000),
    ("3-2", 1),
    ("", 1), ("0-,", 1), (",0-", 1), ("5", 1), ("-5", 1), ("a-b", 1), ("0-1-2", 1), ("1.5-3", 1), ("0--1", 1),
    (",".join(["0-"] * 9), 1),
    ("0-", 0),
])
def test_windows_refused(text, res):
    with pytest.raises(ValueError):
        tracks.parse_windows(text, res)


def test_check_windows():
    assert tracks.check_windows([(0, -1), (3, 3)]).tolist() == [[0, -1], [3, 3]]
    for bad in ([], [(0, -2)], [(-1, 4)], [(5, 4)], [(0, 1, 2)], [(0.0, 1.0)], (0, -1)):
        with pytest.raises(ValueError):
            tracks.check_windows(bad)


# ---- the text lines ---------------------------------------------------------------------------------------------------------
def test_lines_cover_the_covered_bins_in_bed_order():
    s, L, _ = _chromosome()
    L2 = np.concatenate([L, [[3, 15, 18, 2, 2, 1, 1, 3, 1, 1]]]).astype(np.int64)       # chromosome 1 comes last in len_vec
    s2 = np.concatenate([s, [2, 2, 2]])
    ref = R.state_tracks(s2, L2, [(0, -1), (1, 1)], 3)
    for q in (0, 1):
        lines = tracks.track_lines(ref, L2, 50000, q)
        assert lines[0] == "#chrom\tstart\tstop\ttotal\tdominant\tshare\tentropy\tswitch\tstate1\tstate2\tstate3\n"
        cells = [ln.rstrip("\n").split("\t") for ln in lines[1:]]
        assert all(len(c) == 8 + 3 for c in cells)
        assert [(int(c[0]), int(c[1]) // 50000) for c in cells] == [(1, 1), (1, 2), (3, 0), (3, 1), (3, 2), (3, 5), (3, 6)]
        assert all(int(c[2]) - int(c[1]) == 50000 for c in cells)
        for c in cells:
            counts = ref["track_%s" % c[0]][q][int(c[1]) // 50000]
            assert [int(x) for x in c[8:]] == counts.tolist() and int(c[3]) == counts.sum()
            assert int(c[4]) == (int(np.argmax(counts)) + 1 if counts.sum() else 0)
    first = tracks.track_lines(ref, L2, 50000, 0)[1].split("\t")
    assert first[:5] == ["1", "50000", "100000", "2", "3"] and first[5:8] == ["1.000000", "0.000000", "nan"]


# ---- the command line -------------------------------------------------------------------------------------------------------
def _cli(**extra):
    import phylo_hmrf as cli
    return cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", "unused", quiet="1", **extra)


@pytest.mark.parametrize("extra", [
    dict(render="a.mat"),
    dict(segment="m.npz"),
    dict(postprocess="x.mat"),
    dict(compare="a.mat", compare_with="b.mat"),
    dict(compare="a.mat"),
    dict(domains="a.mat"),
    dict(segment="m.npz", ancestral="posterior"),
    dict(ancestral="posterior"),
    dict(save_model="m.npz"),
    dict(profile="1"),
    dict(filter_device="1"),
    dict(tracks_field="top"),
    dict(tracks_dist=""),
    dict(tracks_dist="1-49999"),
    dict(tracks_dist="2000000"),
    dict(tracks_dist=",".join(["0-"] * 9)),
])
def test_cli_refusals(extra):
    with pytest.raises(SystemExit) as e:
        _cli(tracks="a.mat", **extra)
    assert "--tracks" in str(e.value)
    assert not os.path.exists("unused")


def test_cli_parses_the_options_with_their_defaults():
    import phylo_hmrf as cli
    o = cli.parse_args(["--tracks", "a.mat"])
    assert (o.tracks, o.tracks_field, o.tracks_dist) == ("a.mat", "state_vec", "0-")
    o = cli.parse_args(["--tracks", "a.mat", "--tracks_field", "state_vec_smooth", "--tracks_dist", "0-2000000,2000000-"])
    assert (o.tracks_field, o.tracks_dist) == ("state_vec_smooth", "0-2000000,2000000-")
    assert cli.parse_args([]).tracks == ""
    assert cli.check_tracks("", "top", "x", "0", "r.mat", "m.npz", "", "", "", "", "", "0", "0") is None   # off: nothing to refuse
    assert cli.check_tracks("a.mat", "state_vec", "0-2000000,2000000-", "10000", "", "", "", "", "", "", "", "0", "0") == \
        [(0, 200), (200, -1)]


def test_constants_are_the_headers_and_the_sources():
    from phylo_hmrf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert "#define PHMRF_VERSION 127\n" in txt and _lib.ABI_VERSION == 127          # no ABI bump: an entry point only
    assert "PHMRF_API int phmrf_state_tracks(" in txt and txt.count("phmrf_state_tracks") >= 2
    assert len(_lib.SIGNATURES["phmrf_state_tracks"]) == 11
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "tracks.hip")).read()
    assert "TRACKS_GRID_CAP = %d;" % tracks.GRID_CAP in src
    assert "TRACKS_TILE_H = %d;" % tracks.TILE_H in src
    assert "TRACKS_TILE_W = %d;" % tracks.TILE_W in src
    assert '#include "runs.h"' in src
    assert "tracks.hip" in open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "Makefile")).read()
