"""CPU: the pile-up's restatement (tests/pileup_reference.py) on maps worked by hand, and the host side of
phylo_hmrf_amd.pileup: the two anchor readers, the controls, the summaries, the text and the command line."""
import math
import os

import numpy as np
import pytest

from phylo_hmrf_amd import pileup
from tests import pileup_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _states(obs_g):
    """the state each pile cell of one group holds once, -1 for an empty cell"""
    assert obs_g.sum(axis=-1).max() <= 1
    return np.where(obs_g.sum(axis=-1) == 1, obs_g.argmax(axis=-1), -1).tolist()


def _one(labels, H, W, diag, K, w, ci, cj, orient):
    return R.table(labels, H, W, diag, K, w, 1, [0, 1], np.array([ci]), np.array([cj]), np.array([orient]))[0]


# ---- the restatement by hand ------------------------------------------------------------------------------------------------
# 0 1 2 / 3 4 5 / 6 7 8 around its middle: itself, turned by 180 degrees, transposed, and transposed about the other diagonal
@pytest.mark.parametrize("orient,want", [
    (0, [[0, 1, 2], [3, 4, 5], [6, 7, 8]]),
    (1, [[8, 7, 6], [5, 4, 3], [2, 1, 0]]),
    (2, [[0, 3, 6], [1, 4, 7], [2, 5, 8]]),
    (3, [[8, 5, 2], [7, 4, 1], [6, 3, 0]]),
])
def test_three_by_three_by_hand(orient, want):
    assert _states(_one(np.arange(9), 3, 3, False, 9, 1, 1, 1, orient)) == want


# the 4 x 5 map 0 .. 19 around its corner (0, 4): the cells 3 4 / 8 9 are inside, the rest of the window is not
@pytest.mark.parametrize("orient,want", [
    (0, [[-1, -1, -1], [3, 4, -1], [8, 9, -1]]),
    (1, [[-1, 9, 8], [-1, 4, 3], [-1, -1, -1]]),
    (2, [[-1, 3, 8], [-1, 4, 9], [-1, -1, -1]]),
    (3, [[-1, -1, -1], [9, 4, -1], [8, 3, -1]]),
])
def test_four_by_five_corner_by_hand(orient, want):
    assert _states(_one(np.arange(20), 4, 5, False, 20, 1, 0, 4, orient)) == want


def test_diagonal_block_counts_by_hand():
    """nodes (0,0) (0,1) (0,2) (1,1) (1,2) (2,2): the matrix 0 1 2 / 1 0 1 / 2 1 0; the centres (0, 0) and, in the lower
    triangle, (2, 0); the second group is empty"""
    obs = R.table([0, 1, 2, 0, 1, 0], 3, 3, True, 3, 1, 2, [0, 2, 2], np.array([0, 2]), np.array([0, 0]))
    assert obs[0].tolist() == [[[0, 0, 0], [0, 1, 0], [1, 0, 0]],
                               [[0, 0, 0], [1, 0, 1], [0, 2, 0]],
                               [[0, 0, 0], [0, 1, 0], [1, 0, 0]]]
    assert not obs[1].any()
    twice = R.table([0, 1, 2, 0, 1, 0], 3, 3, True, 3, 1, 1, [0, 4], np.array([0, 2, 0, 2]), np.array([0, 0, 0, 0]))
    assert np.array_equal(twice[0], 2 * obs[0])               # a centre given twice counts twice


def test_the_window_may_be_wider_than_the_region_or_miss_it():
    obs = R.table(np.arange(6), 2, 3, False, 6, 3, 1, [0, 1], np.array([0]), np.array([0]))
    assert obs.sum() == 6 and _states(obs[0])[3][3:6] == [0, 1, 2] and _states(obs[0])[4][3:6] == [3, 4, 5]
    for ci, cj in ((-4, 0), (0, -4), (5, 0), (0, 6), (-100, -100)):
        assert not R.table(np.arange(6), 2, 3, False, 6, 3, 1, [0, 1], np.array([ci]), np.array([cj])).any()


def test_a_diagonal_region_is_its_own_mirror():
    rng = np.random.default_rng(1)
    H, K, w = 9, 5, 2
    labels = rng.integers(0, K, H * (H + 1) // 2)
    ci, cj, o = rng.integers(-2, H + 2, 30), rng.integers(-2, H + 2, 30), rng.integers(0, 4, 30)
    a = R.table(labels, H, H, True, K, w, 3, [0, 10, 10, 30], ci, cj, o)
    b = R.table(labels, H, H, True, K, w, 3, [0, 10, 10, 30], cj, ci, o ^ 2)
    assert a.sum() > 0 and np.array_equal(a, b)


def test_the_flip_reverses_both_pile_axes():
    rng = np.random.default_rng(2)
    for H, W, diag in ((7, 7, True), (4, 9, False)):
        labels = rng.integers(0, 6, H * (H + 1) // 2 if diag else H * W)
        ci, cj, o = rng.integers(-1, H + 1, 12), rng.integers(-1, W + 1, 12), rng.integers(0, 4, 12)
        a = R.table(labels, H, W, diag, 6, 2, 2, [0, 5, 12], ci, cj, o)
        b = R.table(labels, H, W, diag, 6, 2, 2, [0, 5, 12], ci, cj, o ^ 1)
        assert np.array_equal(b, a[:, ::-1, ::-1]) and not np.array_equal(a, b)


def test_the_chromosome_restatement_on_one_region_is_the_region_restatement():
    rng = np.random.default_rng(3)
    H, K = 8, 4
    s = rng.integers(0, K, H * (H + 1) // 2)
    L = np.array([[s.size, 0, s.size, H, H, 5, 5, 0, 1, 3]])
    c = np.array([[3, 7, 9, 0, 0], [3, 12, 6, 1, 3], [4, 7, 9, 0, 0]])             # (the last: another chromosome)
    got = R.state_pileup(s, L, c, 2, K, 2)
    want = R.table(s, H, H, True, K, 2, 2, [0, 1, 2], np.array([2, 7]), np.array([4, 1]), np.array([0, 3]))
    assert np.array_equal(got, want) and got.sum() > 0


# ---- the anchor files -------------------------------------------------------------------------------------------------------
# chromosome 1: ten bins; chromosome 2: bins 1 .. 3
LEN_VEC = np.array([[55, 0, 55, 10, 10, 0, 0, 0, 1, 1], [6, 55, 61, 3, 3, 1, 1, 1, 1, 2]], dtype=np.int64)
BED = """# a comment, then a blank line

chr1 0 250 ctcf 0 +
1\t200\t500\tctcf\t7\t-
chr1 950 1000 boundary
chrX 0 100 ctcf . +
chr3 0 100 other
2 100 301 boundary 0 .
chr1 400 401
"""


def _file(tmp_path, text, name="a.bed"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def test_read_anchors(tmp_path):
    got = pileup.read_anchors(_file(tmp_path, BED), LEN_VEC, 100)
    assert got["names"] == ["ctcf", "boundary", "other", "anchor"] and got["skipped_lines"] == 2
    # midpoints 125, 350, 975, 200, 400
    assert got["centres"].tolist() == [[1, 1, 1, 0, 0], [1, 3, 3, 0, 1], [1, 9, 9, 1, 0], [2, 2, 2, 1, 0], [1, 4, 4, 3, 0]]
    assert got["centres"].dtype == np.int64
    empty = pileup.read_anchors(_file(tmp_path, "# nothing\n\n"), LEN_VEC, 100)
    assert empty["centres"].shape == (0, 5) and empty["names"] == [] and empty["skipped_lines"] == 0


def test_read_anchor_pairs(tmp_path):
    text = ("chr1 0 100 chr1 800 900 loop\n"
            "chr1\t700\t900\tchr1\t100\t200\n"                # no name; swapped so that a <= b
            "chr1 0 100 chr2 0 100 loop\n"                    # two chromosomes
            "chr5 0 100 chr5 300 400 other\n"                 # not in the map
            "2 100 200 chr2 250 350 other extra fields\n")
    got = pileup.read_anchor_pairs(_file(tmp_path, text, "a.bedpe"), LEN_VEC, 100)
    assert got["names"] == ["loop", "pair", "other"] and got["skipped_lines"] == 2
    assert got["centres"].tolist() == [[1, 0, 8, 0, 0], [1, 1, 8, 1, 0], [2, 1, 3, 2, 0]]


@pytest.mark.parametrize("text,word", [
    ("chr1 0\n", "expected"), ("chr1 zero 100 A\n", "expected"), ("chr1 0 1e3 A\n", "expected"),
    ("chr1 100 100 A\n", "start"), ("chr1 200 100 A\n", "start"), ("chr1 -5 100 A\n", "negative"),
    ("chr1 0 100 A 0 x\n", "strand"), ("chr1 0 100 A 0 ++\n", "strand"),
    ("".join("chr1 %d %d n%d\n" % (100 * k, 100 * k + 100, k) for k in range(9)), "more than 8 names"),
])
def test_anchors_refused(tmp_path, text, word):
    with pytest.raises(ValueError) as e:
        pileup.read_anchors(_file(tmp_path, text), LEN_VEC, 100)
    assert word in str(e.value) and "line" in str(e.value)


@pytest.mark.parametrize("text,word", [
    ("chr1 0 100 chr1 200\n", "expected"), ("chr1 0 100 chr1 a 300\n", "expected"), ("chr1 0 100 chr1 300 300\n", "start"),
    ("chr1 100 0 chr1 300 400\n", "start"), ("chr1 0 100 chr1 -300 400\n", "negative"),
    ("".join("chr1 0 100 chr1 %d %d n%d\n" % (100 * k, 100 * k + 100, k) for k in range(9)), "more than 8 names"),
])
def test_anchor_pairs_refused(tmp_path, text, word):
    with pytest.raises(ValueError) as e:
        pileup.read_anchor_pairs(_file(tmp_path, text), LEN_VEC, 100)
    assert word in str(e.value) and "line" in str(e.value)


def test_eight_names_are_accepted_and_the_resolution_is_checked(tmp_path):
    text = "".join("chr1 %d %d n%d\n" % (100 * k, 100 * k + 100, k) for k in range(8))
    got = pileup.read_anchors(_file(tmp_path, text), LEN_VEC, 100)
    assert got["centres"][:, 3].tolist() == list(range(8)) and len(got["names"]) == pileup.MAX_NAMES
    assert 2 * pileup.MAX_NAMES == pileup.MAX_GROUPS
    with pytest.raises(ValueError):
        pileup.read_anchors(_file(tmp_path, text), LEN_VEC, 0)


# ---- controls, summaries ----------------------------------------------------------------------------------------------------
def test_with_controls():
    c = np.array([[1, 5, 9, 0, 0], [1, 1, 4, 1, 3], [2, 0, 0, 1, 1]])
    got = pileup.with_controls(c, 2, 2)
    assert got.tolist() == [[1, 5, 9, 0, 0], [1, 1, 4, 1, 3], [2, 0, 0, 1, 1],
                            [1, 3, 7, 2, 0], [1, 7, 11, 2, 0], [1, 3, 6, 3, 3], [2, 2, 2, 3, 1]]     # (-1, 2) and (-2, -2) dropped
    assert np.array_equal((got[:, 2] - got[:, 1])[3:], [4, 4, 3, 0])                                 # the genomic distance is kept
    assert pileup.with_controls(np.zeros((0, 5), dtype=np.int64), 1, 1).shape == (0, 5)
    for bad in (dict(shift_bins=0, G=2), dict(shift_bins=1, G=1), dict(shift_bins=1, G=0)):
        with pytest.raises(ValueError):
            pileup.with_controls(c, **bad)


def test_pile_summary():
    obs = np.array([[[3, 1, 0, 0], [2, 0, 2, 0]], [[0, 0, 0, 0], [0, 0, 0, 5]], [[1, 1, 1, 1], [0, 3, 3, 2]]])
    s = pileup.pile_summary(obs)
    assert s["total"].tolist() == [[4, 4], [0, 5], [4, 8]]
    assert s["dominant"].tolist() == [[0, 0], [-1, 3], [0, 1]]                  # the lowest state on ties, -1 when empty
    assert s["share"].tolist() == [[0.75, 0.5], [0.0, 1.0], [0.25, 0.375]]
    want = [[-(0.75 * math.log2(0.75) + 0.25 * math.log2(0.25)), 1.0], [0.0, 0.0],
            [2.0, -(2 * 0.375 * math.log2(0.375) + 0.25 * math.log2(0.25))]]
    assert np.allclose(s["entropy"], want, rtol=1e-14, atol=0) and s["entropy"][1].tolist() == [0.0, 0.0]


def test_log2_ratio():
    obs = np.array([[2, 2, 0], [1, 0, 0], [0, 0, 0], [1, 1, 0]])
    ctl = np.array([[1, 3, 0], [0, 0, 0], [1, 1, 0], [4, 0, 4]])
    got = pileup.log2_ratio(obs, ctl)
    assert got[0, 0] == np.log2(0.5 / 0.25 + 1e-16) and got[0, 1] == np.log2(0.5 / 0.75 + 1e-16) and np.isnan(got[0, 2])
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all()                   # a total of 0 on either side
    assert got[3, 0] == 0.0 and np.isnan(got[3, 1]) and got[3, 2] == np.log2(1e-16)
    assert np.isnan(pileup.log2_ratio(obs, np.zeros_like(obs))).all()
    with pytest.raises(ValueError):
        pileup.log2_ratio(obs, ctl[:2])


def test_pileup_lines_and_image():
    obs = np.zeros((1, 3, 3, 2), dtype=np.int64)
    obs[0, 0, 0], obs[0, 1, 1], obs[0, 2, 1] = [1, 3], [2, 2], [4, 0]
    ctl = np.zeros_like(obs)
    ctl[0, 0, 0], ctl[0, 1, 1] = [2, 2], [0, 4]
    lines = pileup.pileup_lines(obs, ["ctcf"], 1, 1000, ctl)
    assert lines[0] == "#name\tu_bp\tv_bp\ttotal\tdominant_state\tshare\tentropy_bits\tcontrol_total\tlog2_ratio\tstate_1\tstate_2\n"
    assert len(lines) == 10
    assert lines[1] == "ctcf\t-1000\t-1000\t4\t2\t0.750000\t%.6f\t4\t%.4f\t1\t3\n" % (0.8112781244591328, math.log2(1.5))
    assert lines[2] == "ctcf\t-1000\t0\t0\t0\t0.000000\t0.000000\t0\tnan\t0\t0\n"
    assert lines[5] == "ctcf\t0\t0\t4\t1\t0.500000\t1.000000\t4\tnan\t2\t2\n"          # the control holds no state 1 there
    assert lines[8] == "ctcf\t1000\t0\t4\t1\t1.000000\t0.000000\t0\tnan\t4\t0\n"
    plain = pileup.pileup_lines(obs, ["ctcf"], 1, 1000)
    assert plain[0].count("\t") == 8 and plain[1] == "ctcf\t-1000\t-1000\t4\t2\t0.750000\t0.811278\t1\t3\n"
    palette = np.array([[10, 20, 30], [40, 50, 60]], dtype=np.uint8)
    img = pileup.pile_image(obs[0], palette)
    assert img.shape == (24, 24, 3) and img.dtype == np.uint8
    assert img[0, 0].tolist() == [40, 50, 60] and img[7, 7].tolist() == [40, 50, 60] and img[8, 8].tolist() == [10, 20, 30]
    assert img[0, 8].tolist() == [255, 255, 255] and img[23, 15].tolist() == [10, 20, 30] and img[23, 16].tolist() == [255, 255, 255]


# ---- no GPU, no answer ------------------------------------------------------------------------------------------------------
def test_state_pileup_needs_a_gpu(monkeypatch):
    from phylo_hmrf_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    s = np.zeros(61, dtype=np.int64)
    c = np.array([[1, 2, 3, 0, 0]])
    with pytest.raises(RuntimeError) as e:
        pileup.state_pileup(s, LEN_VEC, c, 2)
    assert "no CPU fallback" in str(e.value)
    for bad in (dict(flank=-1), dict(flank=65), dict(K=65), dict(K=0), dict(G=17), dict(G=0),
                dict(centres=np.array([[1, 2, 3, 1, 0]]), G=1), dict(centres=np.array([[1, 2, 3, -1, 0]])),
                dict(centres=np.array([[1, 2, 3, 0, 4]])), dict(centres=np.array([[1, 2, 3, 0]])),
                dict(centres=np.array([[1.0, 2, 3, 0, 0]]))):
        with pytest.raises(ValueError):
            pileup.state_pileup(s, LEN_VEC, **dict(dict(centres=c, flank=2), **bad))


# ---- the command line -------------------------------------------------------------------------------------------------------
def _cli(**extra):
    import phylo_hmrf as cli
    return cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", "unused", quiet="1", **extra)


@pytest.mark.parametrize("extra", [
    dict(segment="m.npz"),
    dict(postprocess="x.mat"),
    dict(compare="a.mat", compare_with="b.mat"),
    dict(compare_with="b.mat"),
    dict(domains="a.mat"),
    dict(render="a.mat"),
    dict(tracks="a.mat"),
    dict(enrich="a.mat", enrich_bed="a.bed"),
    dict(ancestral="posterior"),
    dict(save_model="m.npz"),
    dict(profile="1"),
    dict(filter_device="1"),
    dict(pileup_field="top"),
    dict(pileup_flank="-50000"),
    dict(pileup_flank="3250000"),                            # 65 bins
    dict(pileup_flank="wide"),
    dict(pileup_shift="75000"),                              # one bin and a half
    dict(pileup_shift="-50000"),
    dict(pileup_bedpe="a.bedpe"),                            # both anchor files
    dict(pileup_bed=""),                                     # neither
    dict(pileup="", pileup_bed="a.bed"),                     # anchors without a map
    dict(pileup="", pileup_bed="", pileup_bedpe="a.bedpe"),
])
def test_cli_refusals(extra):
    with pytest.raises(SystemExit) as e:
        _cli(**dict(dict(pileup="a.mat", pileup_bed="a.bed"), **extra))
    assert "--pileup" in str(e.value)
    assert not os.path.exists("unused")


def test_cli_parses_the_options_with_their_defaults():
    import phylo_hmrf as cli
    o = cli.parse_args(["--pileup", "a.mat", "--pileup_bed", "a.bed"])
    assert (o.pileup, o.pileup_bed, o.pileup_bedpe, o.pileup_field, o.pileup_flank, o.pileup_shift, o.pileup_colors) == \
        ("a.mat", "a.bed", "", "state_vec", "1000000", "0", "")
    o = cli.parse_args(["--pileup", "a.mat", "--pileup_bedpe", "l.bedpe", "--pileup_field", "state_vec_smooth", "--pileup_flank",
                        "500000", "--pileup_shift", "2000000", "--pileup_colors", "c.txt"])
    assert (o.pileup_bedpe, o.pileup_field, o.pileup_flank, o.pileup_shift, o.pileup_colors) == \
        ("l.bedpe", "state_vec_smooth", "500000", "2000000", "c.txt")
    assert cli.parse_args([]).pileup == ""
    off = ("", "top", "x", "y", "7", "s.npz", "p.mat", "c.mat", "d.mat", "r.mat", "t.mat", "e.mat", "posterior", "m.npz", "1", "1")
    assert cli.check_pileup("", "", *off) is None             # off: nothing to refuse
    quiet = ("", "", "", "", "", "", "", "", "", "0", "0")
    assert cli.check_pileup("a.mat", "a.bed", "", "state_vec", "1000000", "0", "50000", *quiet) == (20, 0)
    assert cli.check_pileup("a.mat", "", "a.bedpe", "state_vec_smooth", "99999", "150000", "50000", *quiet) == (1, 3)
    assert cli.check_pileup("a.mat", "a.bed", "", "state_vec", "3200000", "0", "50000", *quiet) == (64, 0)
    assert pileup.check_bins(10000, 0, 10000) == (0, 1)


def test_constants_are_the_headers_and_the_sources():
    from phylo_hmrf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert "#define PHMRF_VERSION 127\n" in txt and _lib.ABI_VERSION == 127          # no ABI bump: an entry point only
    assert "PHMRF_API int phmrf_state_pileup(" in txt
    assert len(_lib.SIGNATURES["phmrf_state_pileup"]) == 13
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "pileup.hip")).read()
    assert "PILEUP_LANES = %d;" % pileup.LANES in src
    assert "PILEUP_CHUNK = %d;" % pileup.CHUNK in src
    assert "PILEUP_GRID_CAP = %d;" % pileup.GRID_CAP in src
    assert "PILEUP_MAX_FLANK = %d;" % pileup.MAX_FLANK in src
    shared = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "interval_lists.h")).read()  # what pileup, query and aggregate compile
    assert "constexpr int MAX_GROUPS = %d;" % pileup.MAX_GROUPS in shared
    assert '#include "interval_lists.h"' in src and '#include "runs.h"' in shared and "getenv" not in src + shared
    mk = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "Makefile")).read()
    assert "pileup.hip" in mk and "interval_lists.h" in mk
