"""CPU: the pair enrichment's restatement (tests/enrich_reference.py) on maps worked by hand, and the host side of
phylo_hmrf_amd.enrich: the annotation reader, the distance-matched expectation, the folding, the text and the command line."""
import math
import os

import numpy as np
import pytest

from phylo_hmrf_amd import enrich
from tests import enrich_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(table, **rows):
    """the table's rows named p<index> hold the given values, every other row is zero"""
    want = np.zeros_like(table)
    for name, values in rows.items():
        want[int(name[1:])] = values
    assert np.array_equal(table, want), (table.tolist(), want.tolist())


# ---- the restatement by hand ------------------------------------------------------------------------------------------------
# a diagonal block of 3 bins, nodes (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); bins 0 and 1 are of class 1 and lie in segment 0
DIAG = dict(labels=[0, 1, 2, 0, 1, 0], H=3, W=3, diag=True, dist0=0, K=3, C=2, row_class=[1, 1, 0], row_seg=[0, 0, -1])
# a 2 x 3 block with dist0 = -1: dist0 + j - i is -1 0 1 / -2 -1 0, so the diagonals -1 and 1 fold onto the distance 1
OFF = dict(labels=[0, 1, 0, 1, 0, 1], H=2, W=3, diag=False, dist0=-1, K=2, C=2, row_class=[1, 0], col_class=[0, 1, 1])


def test_diagonal_block_by_hand():
    obs, sd, cd = R.tables(**DIAG)
    _rows(obs, p7=[2, 1, 0], p4=[0, 1, 1], p0=[1, 0, 0])      # p = (class_i 2 + class_j) 2 + same
    assert sd.tolist() == [[3, 0, 0], [0, 2, 0], [0, 0, 1]]
    _rows(cd.T, p7=[2, 1, 0], p4=[0, 1, 1], p0=[1, 0, 0])
    obs, sd, cd = R.tables(**dict(DIAG, row_seg=None))        # without segments every pair is `same = 0`
    _rows(obs, p6=[2, 1, 0], p4=[0, 1, 1], p0=[1, 0, 0])


def test_a_window_on_the_diagonal_block():
    obs, sd, cd = R.tables(d_min=1, d_max=1, d_lo=1, D=1, **DIAG)
    _rows(obs, p7=[0, 1, 0], p4=[0, 1, 0])
    assert sd.tolist() == [[0, 2, 0]]
    _rows(cd.T, p7=[1], p4=[1])
    obs, sd, cd = R.tables(d_min=5, d_max=-1, d_lo=5, D=0, **DIAG)
    assert not obs.any() and sd.shape == (0, 3) and cd.shape == (0, 8)


def test_off_diagonal_block_whose_diagonals_fold_by_hand():
    obs, sd, cd = R.tables(**OFF)
    _rows(obs, p4=[1, 0], p6=[1, 1], p0=[0, 1], p2=[1, 1])
    assert sd.tolist() == [[0, 2], [3, 0], [0, 1]]
    _rows(cd.T, p6=[1, 1, 0], p2=[1, 1, 0], p4=[0, 1, 0], p0=[0, 0, 1])
    # the state is a function of the distance here: the expectation is the observation
    assert np.array_equal(R.expected(sd, cd), obs) and np.array_equal(enrich.expected(sd, cd), obs)
    obs, sd, cd = R.tables(row_seg=[3, -1], col_seg=[3, -1, 3], **OFF)
    _rows(obs, p5=[1, 0], p6=[0, 1], p7=[1, 0], p0=[0, 1], p2=[1, 1])      # (0, 0) and (0, 2) are inside segment 3; -1 == -1 is not


def test_four_bins_one_class_no_segments():
    labels = [0, 1, 1, 0, 2, 0, 1, 2, 2, 0]
    obs, sd, cd = R.tables(labels, 4, 4, True, 0, 3, 1, [0, 0, 0, 0])
    assert obs.tolist() == [[4, 3, 3], [0, 0, 0]] and np.array_equal(obs[0], sd.sum(axis=0))
    assert cd.tolist() == [[4, 0], [3, 0], [2, 0], [1, 0]]


# ---- the expectation --------------------------------------------------------------------------------------------------------
def _random_region(seed, H, W, diag, dist0, K, C, segments=True):
    rng = np.random.default_rng(seed)
    n = H * (H + 1) // 2 if diag else H * W
    rc, cc = rng.integers(0, C, H), rng.integers(0, C, W)
    rs, cs = (rng.integers(-1, 4, H), rng.integers(-1, 4, W)) if segments else (None, None)
    return dict(labels=rng.integers(0, K, n), H=H, W=W, diag=diag, dist0=dist0, K=K, C=C, row_class=rc, col_class=cc, row_seg=rs,
                col_seg=cs)


@pytest.mark.parametrize("H,W,diag,dist0", [(300, 300, True, 0), (120, 200, False, -60), (90, 40, False, 500)])
def test_expected_keeps_both_margins(H, W, diag, dist0):
    obs, sd, cd = R.tables(**_random_region(H + W, H, W, diag, dist0, 7, 3))
    exp = enrich.expected(sd, cd)
    n = int(obs.sum())
    assert n == (H * (H + 1) // 2 if diag else H * W) == sd.sum() == cd.sum()
    assert np.max(np.abs(exp.sum(axis=1) - obs.sum(axis=1))) <= 1e-9 * n
    assert np.max(np.abs(exp.sum(axis=0) - obs.sum(axis=0))) <= 1e-9 * n
    assert np.allclose(exp, R.expected(sd, cd), rtol=1e-12, atol=1e-9)


def test_a_distance_only_map_has_expected_equal_to_observed():
    reg = _random_region(5, 150, 150, True, 0, 6, 3)
    i, j = R.nodes(150, 150, True)
    reg["labels"] = ((j - i) // 7) % 5                   # (state 5 does not occur: its expectation is 0)
    obs, sd, cd = R.tables(**reg)
    exp = enrich.expected(sd, cd)
    assert np.array_equal(exp, obs.astype(np.float64))
    l2 = enrich.log2_enrichment(obs, exp)
    assert np.all(l2[exp > 0] == np.log2(1.0 + 1e-16)) and np.all(np.isnan(l2[exp == 0])) and (exp == 0).any()


def test_expected_skips_empty_distances_and_checks_its_input():
    sd = np.array([[2, 2], [0, 0], [0, 3]])
    cd = np.array([[1, 3], [0, 0], [3, 0]])
    assert enrich.expected(sd, cd).tolist() == [[0.5, 3.5], [1.5, 1.5]]
    assert enrich.expected(np.zeros((0, 2)), np.zeros((0, 8))).tolist() == np.zeros((8, 2)).tolist()
    with pytest.raises(ValueError):
        enrich.expected(sd, cd[:2])


def test_fold_pairs():
    C, K = 3, 2
    t = np.arange(2 * C * C * K).reshape(2 * C * C, K)
    f = enrich.fold_pairs(t, C)
    o = t.reshape(C, C, 2, K)
    assert f.shape == (C, C, 2, K) and f.sum() == t.sum()
    for a in range(C):
        for b in range(C):
            want = o[a, a] if a == b else (o[a, b] + o[b, a] if a < b else 0 * o[a, b])
            assert np.array_equal(f[a, b], want)
    assert enrich.fold_pairs(np.ones(8), 2).tolist() == [[[1, 1], [2, 2]], [[0, 0], [1, 1]]]
    with pytest.raises(ValueError):
        enrich.fold_pairs(t, 2)


# ---- the distance range -----------------------------------------------------------------------------------------------------
def test_distance_range_against_brute_force():
    shapes = [(1, 1, True), (4, 4, True), (1, 1, False), (1, 5, False), (5, 1, False), (3, 4, False), (6, 2, False)]
    for H, W, diag in shapes:
        for dist0 in ([0] if diag else [0, 1, -1, 2, -3, 5, -7, 40, -40]):
            i, j = R.nodes(H, W, diag)
            d = np.abs(dist0 + j - i)
            for d_min in range(0, 9):
                for d_max in [-1] + list(range(d_min, 10)) + [100]:
                    inside = np.unique(d[(d >= d_min) & ((d <= d_max) if d_max != -1 else True)])
                    got = enrich.distance_range(H, W, diag, dist0, d_min, d_max)
                    if inside.size == 0:
                        assert got is None, (H, W, diag, dist0, d_min, d_max)
                    else:                                    # tight, and without a gap
                        assert got == (inside[0], inside.size) and inside[-1] - inside[0] + 1 == inside.size


# ---- the annotation file ----------------------------------------------------------------------------------------------------
# chromosome 1: ten bins; chromosome 2: bins 1 .. 3
LEN_VEC = np.array([[55, 0, 55, 10, 10, 0, 0, 0, 1, 1], [6, 55, 61, 3, 3, 1, 1, 1, 1, 2]], dtype=np.int64)
BED = """# a comment, then a blank line

chr1 0 250 A
1\t200\t500\tB
chr1 950 1000 A
chrX 0 100 A
chr3 0 100 B
2 0 1000000 B
chr1 100 700 C
"""


def _bed(tmp_path, text):
    path = os.path.join(str(tmp_path), "a.bed")
    with open(path, "w") as fh:
        fh.write(text)
    return path


def test_read_annotation(tmp_path):
    ann = enrich.read_annotation(_bed(tmp_path, BED), LEN_VEC, 100)
    assert ann["names"] == ["none", "A", "B", "C"] and ann["skipped_lines"] == 2 and ann["bin_seg"] is None
    # midpoints 50, 150, ...: [0, 250) holds bins 0 and 1, [200, 500) bins 2 - 4, [950, 1000) bin 9; C comes last and gets
    # what is left of bins 1 - 6
    assert ann["bin_class"][1].tolist() == [1, 1, 2, 2, 2, 3, 3, 0, 0, 1] and ann["bin_class"][1].dtype == np.uint8
    assert ann["bin_class"][2].tolist() == [2, 2, 2, 2] and sorted(ann["bin_class"]) == [1, 2]
    seg = enrich.read_annotation(_bed(tmp_path, BED), LEN_VEC, 100, segments=True)
    assert seg["bin_seg"][1].tolist() == [0, 0, 1, 1, 1, 4, 4, -1, -1, 2] and seg["bin_seg"][1].dtype == np.int32
    assert seg["bin_seg"][2].tolist() == [3, 3, 3, 3]
    assert all(np.array_equal(seg["bin_class"][c], ann["bin_class"][c]) for c in (1, 2))


def test_the_midpoint_decides(tmp_path):
    lv = LEN_VEC[:1]
    got = enrich.read_annotation(_bed(tmp_path, "chr1 150 151 A\nchr1 251 350 B\nchr1 449 450 A\n"), lv, 100)
    assert got["bin_class"][1].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0]      # 150 is in [150, 151); 250 and 450 are in no interval
    got = enrich.read_annotation(_bed(tmp_path, "chr1 0 100000 A\n"), lv, 100)  # beyond the chromosome's bins
    assert got["bin_class"][1].tolist() == [1] * 10


@pytest.mark.parametrize("text,word", [
    ("chr1 0 100\n", "expected"), ("chr1 zero 100 A\n", "expected"), ("chr1 0 1e3 A\n", "expected"),
    ("chr1 100 100 A\n", "start"), ("chr1 200 100 A\n", "start"), ("chr1 -5 100 A\n", "negative"),
    ("".join("chr1 %d %d n%d\n" % (100 * k, 100 * k + 100, k) for k in range(8)), "more than 7 names"),
])
def test_annotation_refused(tmp_path, text, word):
    with pytest.raises(ValueError) as e:
        enrich.read_annotation(_bed(tmp_path, text), LEN_VEC, 100)
    assert word in str(e.value) and "line" in str(e.value)


def test_seven_names_are_accepted(tmp_path):
    text = "".join("chr1 %d %d n%d\n" % (100 * k, 100 * k + 100, k) for k in range(7))
    got = enrich.read_annotation(_bed(tmp_path, text), LEN_VEC, 100)
    assert got["bin_class"][1].tolist() == [1, 2, 3, 4, 5, 6, 7, 0, 0, 0] and len(got["names"]) == enrich.MAX_CLASSES


# ---- the text ---------------------------------------------------------------------------------------------------------------
def test_enrich_lines_on_a_fixed_result():
    obs, exp = np.zeros((8, 2), dtype=np.int64), np.zeros((8, 2))
    obs[2], obs[4], obs[7] = [3, 1], [1, 1], [0, 4]           # (none, A), (A, none), (A, A) inside one segment
    exp[2], exp[4], exp[7] = [2, 2], [1, 1], [1, 3]
    lines = enrich.enrich_lines(dict(obs=obs, expected=exp, K=2, C=2), ["none", "A"])
    assert lines[0] == enrich.HEADER + "\n" and lines[0].count("\t") == 8
    assert lines[1:] == [
        "none\tA\t0\t1\t4\t3.000\t%.4f\t0.666667\t1.000000\n" % math.log2(4 / 3),
        "none\tA\t0\t2\t2\t3.000\t%.4f\t0.333333\t0.333333\n" % math.log2(2 / 3),
        "A\tA\t1\t1\t0\t1.000\t%.4f\t0.000000\t0.000000\n" % math.log2(1e-16),
        "A\tA\t1\t2\t4\t3.000\t%.4f\t1.000000\t0.666667\n" % math.log2(4 / 3),
    ]


# ---- no GPU, no answer ------------------------------------------------------------------------------------------------------
def test_pair_enrichment_needs_a_gpu(monkeypatch):
    from phylo_hmrf_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    s = np.zeros(61, dtype=np.int64)
    with pytest.raises(RuntimeError) as e:
        enrich.pair_enrichment(s, LEN_VEC, {1: np.zeros(10, dtype=np.uint8)})
    assert "no CPU fallback" in str(e.value)
    for bad in (dict(bin_class={1: np.full(10, 8)}), dict(bin_class={1: np.zeros(10)}), dict(bin_class={}, C=9),
                dict(bin_class={}, K=65), dict(bin_class={}, window=(3, 2)), dict(bin_class={}, bin_seg={1: np.full(3, -2)})):
        with pytest.raises(ValueError):
            enrich.pair_enrichment(s, LEN_VEC, **bad)


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
    dict(ancestral="posterior"),
    dict(save_model="m.npz"),
    dict(profile="1"),
    dict(filter_device="1"),
    dict(enrich_field="top"),
    dict(enrich_segments="2"),
    dict(enrich_dist=""),
    dict(enrich_dist="1-49999"),
    dict(enrich_dist="0-2000000,2000000-"),                  # two windows
    dict(enrich_bed=""),
])
def test_cli_refusals(extra):
    with pytest.raises(SystemExit) as e:
        _cli(**dict(dict(enrich="a.mat", enrich_bed="a.bed"), **extra))
    assert "--enrich" in str(e.value)
    assert not os.path.exists("unused")


def test_cli_parses_the_options_with_their_defaults():
    import phylo_hmrf as cli
    o = cli.parse_args(["--enrich", "a.mat", "--enrich_bed", "a.bed"])
    assert (o.enrich, o.enrich_bed, o.enrich_field, o.enrich_dist, o.enrich_segments) == ("a.mat", "a.bed", "state_vec", "0-", "0")
    o = cli.parse_args(["--enrich", "a.mat", "--enrich_bed", "t.bed", "--enrich_field", "state_vec_smooth", "--enrich_dist",
                        "0-2000000", "--enrich_segments", "1"])
    assert (o.enrich_field, o.enrich_dist, o.enrich_segments) == ("state_vec_smooth", "0-2000000", "1")
    assert cli.parse_args([]).enrich == ""
    off = ("", "top", "x", "7", "0", "s.npz", "p.mat", "c.mat", "d.mat", "r.mat", "t.mat", "posterior", "m.npz", "1", "1")
    assert cli.check_enrich("", *off) is None                 # off: nothing to refuse
    with pytest.raises(SystemExit):
        cli.check_enrich("", "a.bed", *off[1:])               # an annotation without a map
    quiet = ("", "", "", "", "", "", "", "", "0", "0")
    assert cli.check_enrich("a.mat", "a.bed", "state_vec", "0-2000000", "1", "10000", *quiet) == (0, 200)
    assert cli.check_enrich("a.mat", "a.bed", "state_vec_smooth", "0-", "0", "50000", *quiet) == (0, -1)


def test_constants_are_the_headers_and_the_sources():
    from phylo_hmrf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert "#define PHMRF_VERSION 127\n" in txt and _lib.ABI_VERSION == 127          # no ABI bump: an entry point only
    assert "PHMRF_API int phmrf_pair_enrichment(" in txt
    assert len(_lib.SIGNATURES["phmrf_pair_enrichment"]) == 19
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "enrich.hip")).read()
    tiles = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "enrich_tiles.h")).read()      # the tile both kernels compile
    assert "ENRICH_GRID_CAP = %d;" % enrich.GRID_CAP in src
    assert "ENRICH_TILE_H = %d;" % enrich.TILE_H in tiles and "ENRICH_TILE_H =" not in src
    assert "ENRICH_TILE_W = %d;" % enrich.TILE_W in tiles and "ENRICH_TILE_W =" not in src
    assert "ENRICH_CHUNK = %d;" % enrich.CHUNK in src
    assert "ENRICH_MAX_CLASSES = %d;" % enrich.MAX_CLASSES in tiles and "ENRICH_MAX_CLASSES =" not in src
    assert '#include "enrich_tiles.h"' in src and '#include "runs.h"' in tiles
    mk = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "Makefile")).read()
    assert "enrich.hip" in mk and "enrich_tiles.h" in mk
