"""CPU: the host side of the rescaled pile-up (phylo_hmrf_amd.aggregate): the axis map by hand, the restatement of
tests/aggregate_reference.py on a map worked by hand and against the references of --query and --pileup, the readers, the
controls, the text columns, the command line's checks and the declaration of phmrf_state_aggregate.  No GPU call is made here."""
import os
import re

import numpy as np
import pytest

from phylo_hmrf_amd import aggregate
from tests import aggregate_reference as R
from tests import pileup_reference, query_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_query_cpu.py's layout: chromosome 1 = two diagonal regions (bins 2 .. 31 and 32 .. 56) and the off-diagonal region
# between them (rows 2 .. 31, columns 32 .. 56); chromosome 2 = one diagonal region (bins 0 .. 11)
SHAPES = [(30, 30, 1, 2, 2, 1), (30, 25, 0, 2, 32, 1), (25, 25, 1, 32, 32, 1), (12, 12, 1, 0, 0, 2)]
K_MAP = 5


def _len_vec(shapes):
    rows, at = [], 0
    for r, (H, W, diag, s1, s2, chrom) in enumerate(shapes):
        n = H * (H + 1) // 2 if diag else H * W
        rows.append([n, at, at + n, H, W, s1, s2, r, diag, chrom])
        at += n
    return np.array(rows, dtype=np.int64), at


def _genome(seed=5):
    L, n = _len_vec(SHAPES)
    return np.random.default_rng(seed).integers(0, K_MAP, n), L


# ---- the axis map by hand ---------------------------------------------------------------------------------------------------
def test_axis_identity():
    lo, hi = aggregate.axis_cells(10, 18, 8, 2)               # n = T: one bin a cell, the flank cells are the neighbouring bins
    assert lo.tolist() == list(range(8, 20)) and hi.tolist() == list(range(9, 21)) and lo.dtype == hi.dtype == np.int64


def test_axis_non_integer_ratio():
    lo, hi = aggregate.axis_cells(100, 120, 8, 0)
    assert (lo - 100).tolist() == [0, 2, 5, 7, 10, 12, 15, 17] and (hi - 100).tolist() == [2, 5, 7, 10, 12, 15, 17, 20]


def test_axis_upsampling():
    lo, hi = aggregate.axis_cells(0, 3, 8, 0)
    assert lo.tolist() == [0, 0, 0, 1, 1, 1, 2, 2] and hi.tolist() == [1, 1, 1, 2, 2, 2, 3, 3]


def test_axis_left_flank_is_a_true_floor():
    lo, hi = aggregate.axis_cells(10, 13, 8, 2)               # edge(0) = 10 + floor(-6 / 8) = 9, not 10 + trunc(-0.75) = 10
    assert lo[:3].tolist() == [9, 9, 10] and hi[:3].tolist() == [10, 10, 11]
    lo, hi = aggregate.axis_cells(0, 5, 2, 1)                 # floor(-5 / 2) = -3
    assert lo.tolist() == [-3, 0, 2, 5] and hi.tolist() == [0, 2, 5, 7]


@pytest.mark.parametrize("T,F", ((1, 0), (2, 1), (8, 4), (7, 3), (64, 32)))
def test_axis_body_spans_the_interval(T, F):
    for x0 in (0, 11):
        for n in (1, 2, T - 1, T, T + 1, 3 * T + 2, 1000):
            if n < 1:
                continue
            lo, hi = aggregate.axis_cells(x0, x0 + n, T, F)
            assert lo.shape == hi.shape == (T + 2 * F,) and np.all(hi > lo) and np.all(np.diff(lo) >= 0)
            body_lo, body_hi = lo[F:F + T], hi[F:F + T]
            assert body_lo[0] == x0 and body_hi.max() == x0 + n and body_lo.min() >= x0
            if n >= T:                                        # the body cells tile [x0, x1)
                assert np.array_equal(body_hi[:-1], body_lo[1:]) and body_hi[-1] == x0 + n
            else:                                             # single bins, in order, every bin of the interval at least once
                assert np.all(body_hi == body_lo + 1) and sorted(set(body_lo.tolist())) == list(range(x0, x0 + n))
    for bad in ((5, 5, 4, 1), (5, 4, 4, 1), (0, 4, 0, 1), (0, 4, 4, -1)):
        with pytest.raises(ValueError):
            aggregate.axis_cells(*bad)


def test_the_kernels_edge_arithmetic_is_the_floor():
    """csrc/aggregate.hip forms (c - F) n / T as (c - F) qn + floor((c - F) rn / T) with n = qn T + rn, and the floor of the
    small second numerator x in [-32 * 63, 96 * 63] as ((x + 32 T) M >> 24) - 32, M = ceil(2^24 / T): exact, and below 2^32"""
    for T in range(1, 65):
        M = ((1 << 24) + T - 1) // T
        x = np.arange(-32 * (T - 1), 96 * (T - 1) + 1, dtype=np.int64)
        assert np.all((x + 32 * T) * M < 1 << 32) and np.array_equal((((x + 32 * T) * M) >> 24) - 32, x // T), T
    for T, F, x0, n in ((8, 4, 10, 3), (7, 3, -50, 1000003), (64, 32, 5, (1 << 30) + 17), (1, 32, 0, (1 << 31) - 1), (33, 0, 7, 32)):
        qn, rn, M = n // T, n % T, ((1 << 24) + T - 1) // T
        d = np.arange(-F, T + F + 1, dtype=np.int64)
        edge = x0 + d * qn + ((((d * rn + 32 * T) * M) >> 24) - 32)
        lo, hi = aggregate.axis_cells(x0, x0 + n, T, F)
        assert np.array_equal(edge[:-1], lo) and np.array_equal(np.maximum(edge[:-1] + 1, edge[1:]), hi)


# ---- the reference on a map worked by hand ----------------------------------------------------------------------------------
HAND = [[0, 1, 0, 0, 2, 2],
        [9, 0, 0, 0, 2, 2],
        [9, 9, 0, 0, 0, 0],
        [9, 9, 9, 1, 1, 1],
        [9, 9, 9, 9, 1, 1],
        [9, 9, 9, 9, 9, 1]]                                   # the upper triangle of one 6 x 6 diagonal region (9: not stored)


def test_reference_on_a_map_worked_by_hand():
    L, n = _len_vec([(6, 6, 1, 0, 0, 1)])
    s = np.array(HAND)[np.triu_indices(6)]
    assert n == 21 and s.max() == 2
    # feature 0: A = B = [0, 4) at T = 2, F = 1: the cells are [-2, 0), [0, 2), [2, 4), [4, 6); row and column 0 lie before the
    # chromosome's start.  Cell (1, 1) holds (0, 0), (0, 1), (1, 1) and (0, 1) once more for (1, 0): states 0 1 0 1, a tie.
    # feature 1: A = [0, 2), B = [3, 5), flipped: single bins, cell u' of A is bin u' - 1 and cell v' of B is bin v' + 2, and
    # pile cell (u, v) reads (u', v') = (3 - u, 3 - v); its last row is bin -1
    features = [[1, 0, 4, 0, 4, 0, 0], [1, 0, 2, 3, 5, 1, 1]]
    cells, votes = R.state_aggregate(s, L, features, 2, 1, 3, 2)
    z = [0, 0, 0]
    assert cells[0].tolist() == [[z, z, z, z],
                                 [z, [2, 2, 0], [4, 0, 0], [0, 0, 4]],
                                 [z, [4, 0, 0], [3, 1, 0], [2, 2, 0]],
                                 [z, [0, 0, 4], [2, 2, 0], [0, 4, 0]]]
    one = lambda k: [int(k == 0), int(k == 1), int(k == 2)]
    assert votes[0].tolist() == [[z, z, z, z],
                                 [z, one(0), one(0), one(2)],              # (1, 1): the tie goes to state 0
                                 [z, one(0), one(0), one(0)],              # (2, 3): a tie again
                                 [z, one(2), one(0), one(1)]]
    want = [[one(0), one(0), one(0), one(0)],                              # bin 2 against bins 5, 4, 3, 2
            [one(2), one(2), one(0), one(0)],                              # bin 1
            [one(2), one(2), one(0), one(0)],                              # bin 0
            [z, z, z, z]]                                                  # bin -1
    assert cells[1].tolist() == want and votes[1].tolist() == want


# ---- identities on seeded maps ----------------------------------------------------------------------------------------------
def test_body_cells_against_the_query_reference():
    """A = B and n >= T: the body cells tile A x A, so their `cells` sum to 2 (the query's counts) - (the diagonal nodes in A)"""
    s, L = _genome()
    T, F = 3, 1
    for chrom, a0, a1 in ((1, 5, 20), (1, 25, 40), (1, 0, 60), (1, 30, 33), (2, 0, 12), (2, 4, 9)):
        inside = query_reference.state_query(s, L, [[chrom, a0, a1, a0, a1]], K_MAP)[0][0]
        singles = [[chrom, p, p + 1, p, p + 1] for p in range(a0, a1)]
        on_diagonal = query_reference.state_query(s, L, singles, K_MAP)[0].sum(axis=0)
        for flip in (0, 1):
            cells = R.state_aggregate(s, L, [[chrom, a0, a1, a0, a1, 0, flip]], T, F, K_MAP, 1)[0][0]
            assert np.array_equal(cells[F:F + T, F:F + T].sum(axis=(0, 1)), 2 * inside - on_diagonal), (chrom, a0, a1)


@pytest.mark.parametrize("T,F", ((5, 2), (1, 3), (7, 0)))
def test_single_bin_cells_against_the_pileup_reference(T, F):
    """T odd, n = T, no flip: cells == votes == the pile of tests/pileup_reference.py around a0 + (T - 1) / 2, w = F + (T - 1) / 2"""
    s, L = _genome(6)
    h = (T - 1) // 2
    features = [[1, a, a + T, a, a + T, t & 1, 0] for t, a in enumerate((0, 2, 27, 30, 33, 50, 55))] + [[1, 10, 10 + T, 36, 36 + T, 0, 0]]
    features += [[2, a, a + T, a, a + T, 1, 0] for a in (0, 5, 9)]
    centres = [[f[0], f[1] + h, f[3] + h, f[5], 0] for f in features]
    cells, votes = R.state_aggregate(s, L, features, T, F, K_MAP, 2)
    pile = pileup_reference.state_pileup(s, L, centres, F + h, K_MAP, 2)
    assert np.array_equal(cells, pile) and np.array_equal(votes, pile) and pile.any()


def test_flipping_reverses_both_axes_and_votes_are_bounded():
    s, L = _genome(7)
    features = np.array([[1, 3, 30, 3, 30, 0, 0], [1, 28, 36, 28, 36, 1, 0], [1, 0, 9, 40, 57, 0, 0], [2, 1, 4, 1, 4, 1, 0],
                         [1, 3, 30, 3, 30, 0, 0]], dtype=np.int64)
    flipped = features.copy()
    flipped[:, 6] = 1
    for T, F in ((4, 2), (5, 0)):
        cells, votes = R.state_aggregate(s, L, features, T, F, K_MAP, 2)
        cells_f, votes_f = R.state_aggregate(s, L, flipped, T, F, K_MAP, 2)
        assert np.array_equal(cells_f, cells[:, ::-1, ::-1]) and np.array_equal(votes_f, votes[:, ::-1, ::-1]) and votes.any()
        assert np.all(votes.sum(axis=-1) <= np.array([3, 2])[:, None, None]) and votes.sum(axis=-1).max() == 3
        assert np.all((votes.sum(axis=-1) > 0) == (cells.sum(axis=-1) > 0))


# ---- the readers ------------------------------------------------------------------------------------------------------------
def _write(tmp_path, name, text):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def test_read_features(tmp_path):
    _, L = _genome()
    bed = _write(tmp_path, "tads.bed", "# a comment\n\nchr1 100 250 tad 0 +\n1\t200\t300\ttad\t0\t-\nchr1 0 100\nchr2 150 151 border 0 .\n"
                 "chr7 0 100 tad\nchrX 0 100 other\nchr1 40 60 tad\nchr1 300 300 tad\n")
    read = aggregate.read_features(bed, L, 100)
    # the bin rule: every bin the interval overlaps, at least one
    assert read["features"].tolist() == [[1, 1, 3, 1, 3, 0, 0], [1, 2, 3, 2, 3, 0, 1], [1, 0, 1, 0, 1, 1, 0], [2, 1, 2, 1, 2, 2, 0],
                                         [1, 0, 1, 0, 1, 0, 0], [1, 3, 4, 3, 4, 0, 0]]
    assert read["names"] == ["tad", "feature", "border", "other"] and read["skipped_lines"] == 2 and read["skipped_short"] == 0
    short = aggregate.read_features(bed, L, 100, min_bp=100)
    assert short["features"].tolist() == [[1, 1, 3, 1, 3, 0, 0], [1, 2, 3, 2, 3, 0, 1], [1, 0, 1, 0, 1, 1, 0]]
    assert short["skipped_short"] == 3 and short["skipped_lines"] == 2 and short["names"] == read["names"]
    assert aggregate.read_features(_write(tmp_path, "none.bed", "# nothing\n"), L, 100)["features"].shape == (0, 7)
    for text in ("chr1 100\n", "chr1 a 200\n", "chr1 300 200\n", "chr1 -5 200\n", "chr1 100 200 tad 0 x\n",
                 "".join("chr1 0 100 n%d\n" % t for t in range(9))):
        with pytest.raises(ValueError):
            aggregate.read_features(_write(tmp_path, "bad.bed", text), L, 100)


def test_read_feature_pairs(tmp_path):
    _, L = _genome()
    bedpe = _write(tmp_path, "pairs.bedpe", "chr1 100 250 chr1 1000 1300 pair_a\nchr1 1000 1300 chr1 100 250 pair_a\nchr1 0 50 chr1 0 50\n"
                   "chr1 0 100 chr2 0 100 pair_a\nchr9 0 100 chr9 0 100\nchr2 500 700 chr2 100 120 pair_b\n")
    read = aggregate.read_feature_pairs(bedpe, L, 100)
    assert read["features"].tolist() == [[1, 1, 3, 10, 13, 0, 0], [1, 1, 3, 10, 13, 0, 0], [1, 0, 1, 0, 1, 1, 0], [2, 1, 2, 5, 7, 2, 0]]
    assert read["names"] == ["pair_a", "pair", "pair_b"] and read["skipped_lines"] == 2 and read["skipped_short"] == 0
    short = aggregate.read_feature_pairs(bedpe, L, 100, min_bp=100)
    assert short["features"].tolist() == [[1, 1, 3, 10, 13, 0, 0], [1, 1, 3, 10, 13, 0, 0]] and short["skipped_short"] == 2
    for text in ("chr1 100 200 chr1 300\n", "chr1 100 200 chr1 x 400\n", "chr1 200 100 chr1 300 400\n"):
        with pytest.raises(ValueError):
            aggregate.read_feature_pairs(_write(tmp_path, "bad.bedpe", text), L, 100)


# ---- controls, the text, the checks of the arguments ------------------------------------------------------------------------
def test_with_controls():
    features = [[1, 10, 20, 10, 20, 0, 1], [1, 2, 5, 30, 40, 1, 0], [2, 0, 4, 0, 4, 0, 0]]
    got = aggregate.with_controls(features, 3, 2)
    assert got.tolist() == features + [[1, 7, 17, 7, 17, 2, 1], [1, 13, 23, 13, 23, 2, 1], [1, 5, 8, 33, 43, 3, 0], [2, 3, 7, 3, 7, 2, 0]]
    assert aggregate.with_controls(np.zeros((0, 7), dtype=np.int64), 3, 1).shape == (0, 7)
    for shift, G in ((0, 2), (3, 1), (3, 0)):
        with pytest.raises(ValueError):
            aggregate.with_controls(features, shift, G)


def test_the_text_columns():
    votes, cells = np.array([[[[3, 1]]], [[[0, 0]]]]), np.array([[[[10, 2]]], [[[0, 0]]]])
    plain = aggregate.aggregate_lines(votes, cells, ["tad", "gap"], 1, 0)
    assert plain[0] == "#name\tu\tv\tu_pos\tv_pos\tfeatures\tdominant_state\tshare\tentropy_bits\tbin_pairs\tstate_1\tstate_2\n"
    assert plain[1] == "tad\t0\t0\t0.5000\t0.5000\t4\t1\t0.750000\t0.811278\t12\t3\t1\n"
    assert plain[2] == "gap\t0\t0\t0.5000\t0.5000\t0\t0\t0.000000\t0.000000\t0\t0\t0\n" and len(plain) == 3
    ctl = aggregate.aggregate_lines(votes, cells, ["tad", "gap"], 1, 0, ctl_votes=np.array([[[[1, 1]]], [[[2, 0]]]]))
    assert ctl[0].split("\t")[10:12] == ["control_features", "log2_ratio"]
    assert ctl[1] == "tad\t0\t0\t0.5000\t0.5000\t4\t1\t0.750000\t0.811278\t12\t2\t0.5850\t3\t1\n" and ctl[2].split("\t")[10:12] == ["2", "nan"]
    grid = aggregate.aggregate_lines(np.zeros((1, 4, 4, 2), dtype=np.int64), np.zeros((1, 4, 4, 2), dtype=np.int64), ["tad"], 2, 1)
    assert len(grid) == 17 and [ln.split("\t")[3] for ln in grid[1::4]] == ["-0.2500", "0.2500", "0.7500", "1.2500"]


def test_state_aggregate_checks_its_arguments():
    s, L = _genome()
    ok = [[1, 5, 9, 5, 9, 0, 0]]
    bad = (dict(features=[[1, 5, 5, 5, 9, 0, 0]]), dict(features=[[1, 5, 9, 9, 5, 0, 0]]), dict(features=[[1, 5, 9, 5, 9, 0, 2]]),
           dict(features=[[1, 5, 9, 5, 9, -1, 0]]), dict(features=[[1, 5, 1 << 30, 5, 9, 0, 0]]), dict(features=[[1, 5, 9, 5, 9, 0]]),
           dict(features=np.array(ok, dtype=np.float64)), dict(body=0), dict(body=65), dict(flank=-1), dict(flank=33), dict(K=0),
           dict(K=65), dict(G=0), dict(G=17), dict(features=[[1, 5, 9, 5, 9, 3, 0]], G=3))
    for change in bad:
        args = dict(features=ok, body=4, flank=2, K=K_MAP, G=None)
        args.update(change)
        with pytest.raises(ValueError):
            aggregate.state_aggregate(s, L, args["features"], args["body"], args["flank"], K=args["K"], G=args["G"])
    assert 16 * (64 + 2 * 32) ** 2 * 64 == aggregate.MAX_TABLE        # the largest table the other limits allow is at the limit


def test_no_gpu_is_an_error():
    from phylo_hmrf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libphmrf.so not built")
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    s, L = _genome()
    with pytest.raises(RuntimeError):
        aggregate.state_aggregate(s, L, [[1, 5, 9, 5, 9, 0, 0]], 4, 2)


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_check_aggregate():
    import phylo_hmrf as cli
    rest = ("", "", "", "", "", "", "", "", "", "", "", "", "0", "0")   # segment .. filter_device
    off = ("state_vec", "32", "16", "0", "0", "")
    assert cli.check_aggregate("", "", "", *off, "50000", *rest) is None
    assert cli.check_aggregate("m.mat", "a.bed", "", *off, "50000", *rest) == (32, 16, 0, 0)
    assert cli.check_aggregate("m.mat", "", "a.bedpe", "state_vec_smooth", "64", "0", "150000", "20000", "c.txt", "50000", *rest) == (64, 0, 3, 20000)
    for args in (("", "a.bed", "") + off, ("", "", "a.bedpe") + off, ("m.mat", "", "") + off, ("m.mat", "a.bed", "b.bedpe") + off,
                 ("m.mat", "a.bed", "", "conf", "32", "16", "0", "0", ""), ("m.mat", "a.bed", "", "state_vec", "0", "16", "0", "0", ""),
                 ("m.mat", "a.bed", "", "state_vec", "65", "16", "0", "0", ""), ("m.mat", "a.bed", "", "state_vec", "32", "33", "0", "0", ""),
                 ("m.mat", "a.bed", "", "state_vec", "32", "-1", "0", "0", ""), ("m.mat", "a.bed", "", "state_vec", "32", "16", "70000", "0", ""),
                 ("m.mat", "a.bed", "", "state_vec", "32", "16", "-50000", "0", ""), ("m.mat", "a.bed", "", "state_vec", "32", "16", "0", "-1", ""),
                 ("m.mat", "a.bed", "", "state_vec", "x", "16", "0", "0", ""),
                 # the sub-options without --aggregate
                 ("", "", "", "state_vec_smooth", "32", "16", "0", "0", ""), ("", "", "", "state_vec", "8", "16", "0", "0", ""),
                 ("", "", "", "state_vec", "32", "4", "0", "0", ""), ("", "", "", "state_vec", "32", "16", "50000", "0", ""),
                 ("", "", "", "state_vec", "32", "16", "0", "10", ""), ("", "", "", "state_vec", "32", "16", "0", "0", "c.txt")):
        with pytest.raises(SystemExit):
            cli.check_aggregate(*args, "50000", *rest)
    names = ("segment", "postprocess", "compare", "domains", "render", "tracks", "enrich", "pileup", "consensus", "query", "ancestral",
             "save_model", "profile", "filter_device")
    for at, name in enumerate(names):
        other = list(rest)
        other[at] = "1" if name in ("profile", "filter_device") else "x.mat"
        with pytest.raises(SystemExit) as e:
            cli.check_aggregate("m.mat", "a.bed", "", *off, "50000", *other)
        assert "--aggregate cannot be combined with --%s" % name in str(e.value)
    opts = cli.parse_args(["--aggregate", "m.mat", "--aggregate_bed", "t.bed", "--aggregate_body", "48"])
    assert (opts.aggregate, opts.aggregate_bed, opts.aggregate_bedpe, opts.aggregate_field, opts.aggregate_body, opts.aggregate_flank,
            opts.aggregate_shift, opts.aggregate_min, opts.aggregate_colors) == ("m.mat", "t.bed", "", "state_vec", "48", "16", "0", "0", "")


def test_every_other_mode_refuses_aggregate():
    import phylo_hmrf as cli
    calls = {
        "profile": (cli.check_profile, ("1", "0.25,0.5", "", "")),
        "compare": (cli.check_compare, ("a.mat", "b.mat", "state_vec", "0", "", "", "", "", "0")),
        "domains": (cli.check_domains, ("a.mat", "state_vec", "", "", "", "", "", "0", "0")),
        "render": (cli.check_render, ("a.mat", "state_vec", "512", "0", "0", "", "", "", "", "", "", "0", "0")),
        "tracks": (cli.check_tracks, ("a.mat", "state_vec", "0-", "50000", "", "", "", "", "", "", "", "0", "0")),
        "enrich": (cli.check_enrich, ("a.mat", "a.bed", "state_vec", "0-", "0", "50000", "", "", "", "", "", "", "", "", "0", "0")),
        "pileup": (cli.check_pileup, ("a.mat", "a.bed", "", "state_vec", "100000", "0", "50000", "", "", "", "", "", "", "", "", "", "0", "0")),
        "consensus": (cli.check_consensus, ("a.mat,b.mat", "state_vec", "0", "-1", "-1", "", "", "", "", "", "", "", "", "", "", "0", "0")),
        "query": (cli.check_query, ("a.mat", "a.bed", "", "state_vec", "0", "50000", "", "", "", "", "", "", "", "", "", "", "", "0", "0")),
    }
    for name, (check, args) in calls.items():
        check(*args)                                          # fine without --aggregate, refused with it
        with pytest.raises(SystemExit) as e:
            check(*args, aggregate="m.mat")
        assert "--aggregate" in str(e.value), name


def test_the_entry_point_is_declared():
    from phylo_hmrf_amd import _lib
    header = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert "#define PHMRF_VERSION 127\n" in header and _lib.ABI_VERSION == 127          # no ABI bump: an entry point only
    m = re.search(r"PHMRF_API int phmrf_state_aggregate\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S)
    assert m and len(m.group(1).split(",")) == 14 == len(_lib.SIGNATURES["phmrf_state_aggregate"])
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "aggregate.hip")).read()
    shared = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "interval_lists.h")).read()  # what pileup, query and aggregate compile
    for name, value in (("AGG_LANES", aggregate.LANES), ("AGG_CHUNK", aggregate.CHUNK), ("AGG_GRID_CAP", aggregate.GRID_CAP),
                        ("AGG_SMALL_AREA", aggregate.SMALL_AREA), ("AGG_WAVES", aggregate.WAVES), ("AGG_WAVE_GRID_CAP", aggregate.WAVE_GRID_CAP),
                        ("AGG_MAX_BODY", aggregate.MAX_BODY), ("AGG_MAX_FLANK", aggregate.MAX_FLANK), ("AGG_MAX_REGIONS", aggregate.MAX_REGIONS)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name
    assert re.search(r"constexpr int MAX_GROUPS = %d;" % aggregate.MAX_GROUPS, shared) and '#include "interval_lists.h"' in src
    assert "constexpr int64_t AGG_MAX_TABLE = (int64_t)1 << 24;" in src and aggregate.MAX_TABLE == 1 << 24
    assert "constexpr int COORD_LIMIT = 1 << 30;" in shared and aggregate.COORD_LIMIT == 1 << 30
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", src + shared))  # integers only
    assert "PHMRF_DETERMINISTIC" not in src + shared and "asm" not in re.sub(r"//.*", "", src + shared)
    assert "aggregate.hip" in open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "Makefile")).read()
    assert aggregate.is_small(32, 32, 2) and not aggregate.is_small(33, 32, 2) and aggregate.is_small(1, 1, 64)
