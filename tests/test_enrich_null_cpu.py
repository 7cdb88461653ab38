"""CPU: the restatement of the enrichment's permutation null (tests/enrich_null_reference.py) against the identities it must
keep, and the host side of phylo_hmrf_amd.enrich's null: the weights, the fixed-point expectation, the shifts, the statistics,
the kernels' group size, the text and the command line."""
import math
import os

import numpy as np
import pytest

from phylo_hmrf_amd import enrich
from tests import enrich_null_reference as N
from tests import enrich_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 24


def _region(seed, H, W, diag, K, C, B, segments=True):
    rng = np.random.default_rng(seed)
    n = H * (H + 1) // 2 if diag else H * W
    cls = np.repeat(rng.integers(0, C, B // 3 + 1), rng.integers(1, 6, B // 3 + 1))[:B]
    seg = np.repeat(rng.integers(-1, 5, B // 3 + 1), rng.integers(1, 6, B // 3 + 1))[:B] if segments else None
    return rng.integers(0, K, n), cls, seg


# ---- the restatement's identities -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,diag,row0,col0,B", [(40, 40, True, 5, 5, 60), (20, 35, False, 3, 41, 80), (30, 30, True, 0, 0, 30)])
def test_shift_zero_is_the_enrichment_and_shifts_are_circular(H, W, diag, row0, col0, B):
    K, C = 5, 3
    labels, cls, seg = _region(H + W, H, W, diag, K, C, B)
    obs0, sd, cd = R.tables(labels, H, W, diag, col0 - row0, K, C, cls[row0:row0 + H], cls[col0:col0 + W], seg[row0:row0 + H],
                            seg[col0:col0 + W])
    w = N.weights(sd)
    for window in ((0, -1), (2, 25)):
        o0, s0, c0 = R.tables(labels, H, W, diag, col0 - row0, K, C, cls[row0:row0 + H], cls[col0:col0 + W], seg[row0:row0 + H],
                              seg[col0:col0 + W], window[0], window[1], 0, sd.shape[0])
        ww = N.weights(s0)
        obs, exq = N.tables(labels, H, W, diag, row0, col0, K, C, cls, seg, B, [0, 7, B + 7, B - 1, 2 * B - 1], ww, window[0], window[1])
        assert np.array_equal(obs[0], o0) and np.array_equal(exq[0], N.expq(c0, ww))
        assert np.array_equal(obs[1], obs[2]) and np.array_equal(exq[1], exq[2])          # s and s + B
        assert np.array_equal(obs[3], obs[4]) and np.array_equal(exq[3], exq[4])
        assert o0.any() and not np.array_equal(obs[0], obs[1])
        assert all(int(o.sum()) == int(o0.sum()) for o in obs)                            # a shift moves no node out of the window
    assert np.array_equal(obs0.sum(axis=0), sd.sum(axis=0)) and all(int(x) <= ONE for x in w.reshape(-1))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_fixed_point_expectation_lies_just_below_the_float_one(seed):
    """0 <= expected ONE - expq <= sum_d Cat[d][p], up to the float's rounding"""
    H, W, K, C = 60, 90, 7, 3
    labels, cls, seg = _region(seed, H, W, False, K, C, 200)
    obs, sd, cd = R.tables(labels, H, W, False, 70, K, C, cls[10:10 + H], cls[80:80 + W], seg[10:10 + H], seg[80:80 + W])
    w = N.weights(sd)
    q = N.expq(cd, w).astype(np.float64)
    gap = R.expected(sd, cd) * ONE - q
    slack = 1e-9 * ONE * max(1, int(cd.sum()))                  # float64 rounding of a sum of at most cd.sum() bin pairs
    assert np.all(gap >= -slack) and np.all(gap <= cd.sum(axis=0)[:, None] + slack)
    assert np.array_equal(enrich.weights(sd), w.astype(np.uint32)) and enrich.weights(sd).dtype == np.uint32
    assert np.array_equal(enrich.expected_fixed(cd, enrich.weights(sd)), N.expq(cd, w))
    assert enrich.expected_fixed(cd, enrich.weights(sd)).dtype == np.int64


def test_a_distance_only_map_has_no_excess_under_any_shift():
    H, W, K, C, B = 50, 50, 6, 3, 70
    _, cls, seg = _region(9, H, W, True, K, C, B)
    i, j = R.nodes(H, W, True)
    labels = ((j - i) // 4) % 5
    _, sd, _ = R.tables(labels, H, W, True, 0, K, C, cls[8:8 + H], None, seg[8:8 + H], None)
    obs, exq = N.tables(labels, H, W, True, 8, 8, K, C, cls, seg, B, [0, 1, 13, B - 1], N.weights(sd))
    assert np.array_equal(obs * ONE, exq) and obs.any()


# ---- the weights and the expectation ----------------------------------------------------------------------------------------
def test_weights_by_hand():
    w = enrich.weights(np.array([[0, 0, 0], [0, 5, 0], [1, 2, 0], [2, 2, 4]]))
    assert w.dtype == np.uint32 and w.shape == (4, 3)
    assert w.tolist() == [[0, 0, 0], [0, ONE, 0], [ONE // 3, (2 * ONE) // 3, 0], [ONE // 4, ONE // 4, ONE // 2]]
    assert w[2].sum() == ONE - 1                                 # floors: a row sums to at most ONE
    assert enrich.weights(np.zeros((0, 4), dtype=np.int64)).shape == (0, 4) and enrich.WEIGHT_ONE == ONE
    from phylo_hmrf_amd import maps
    assert float(enrich.WEIGHT_ONE) == maps.CONF_ONE
    for bad in (np.zeros(3, dtype=np.int64), np.zeros((2, 2)), np.array([[1, -1]])):
        with pytest.raises(ValueError):
            enrich.weights(bad)


def test_expected_fixed_by_hand():
    cd = np.array([[1, 3], [0, 0], [3, 0]])
    w = enrich.weights(np.array([[2, 2], [0, 0], [0, 3]]))
    assert enrich.expected_fixed(cd, w).tolist() == [[ONE // 2, ONE // 2 + 3 * ONE], [3 * (ONE // 2), 3 * (ONE // 2)]]
    assert enrich.expected_fixed(np.zeros((0, 8), dtype=np.int64), np.zeros((0, 2), dtype=np.uint32)).tolist() == [[0, 0]] * 8
    with pytest.raises(ValueError):
        enrich.expected_fixed(cd, w[:2])
    with pytest.raises(ValueError):
        enrich.expected_fixed(cd.astype(np.float64), w)


# ---- the shifts -------------------------------------------------------------------------------------------------------------
# chromosome 1: 135 bins, chromosome 2: 70, chromosome 5: one bin
LEN_VEC = np.array([[2485, 0, 2485, 70, 70, 0, 0, 0, 1, 1], [3150, 2485, 5635, 70, 45, 0, 90, 1, 0, 1],
                    [561, 5635, 6196, 33, 33, 4, 4, 2, 1, 2], [660, 6196, 6856, 33, 20, 4, 50, 3, 0, 2],
                    [1, 6856, 6857, 1, 1, 0, 0, 4, 1, 5]], dtype=np.int64)


def test_draw_shifts():
    a = enrich.draw_shifts(LEN_VEC, 500, min_shift=20, seed=4)
    b = enrich.draw_shifts(LEN_VEC, 500, min_shift=20, seed=4)
    assert sorted(a) == [1, 2, 5] and all(a[c].dtype == np.int64 and a[c].shape == (500,) for c in a)
    assert all(np.array_equal(a[c], b[c]) for c in a)
    assert not np.array_equal(a[1], enrich.draw_shifts(LEN_VEC, 500, min_shift=20, seed=5)[1])
    assert a[1].min() >= 20 and a[1].max() <= 135 - 20 and a[2].min() >= 20 and a[2].max() <= 70 - 20
    assert len(np.unique(a[1])) > 60 and not a[5].any()         # B = 1: the only shift is 0
    # the draws are default_rng(seed)'s, chromosome after chromosome in ascending order
    rng = np.random.default_rng(4)
    assert np.array_equal(a[1], rng.integers(20, 116, 500)) and np.array_equal(a[2], rng.integers(20, 51, 500))
    wide = enrich.draw_shifts(LEN_VEC, 300, min_shift=1000, seed=0)          # m = B // 2: [35, 35] and [67, 68]
    assert set(wide[2].tolist()) == {35} and set(wide[1].tolist()) == {67, 68}
    free = enrich.draw_shifts(LEN_VEC, 4000, seed=1)[2]                      # m = 0: [0, B] mod B
    assert free.min() == 0 and free.max() == 69
    for bad in (dict(n=0), dict(n=3, min_shift=-1)):
        with pytest.raises(ValueError):
            enrich.draw_shifts(LEN_VEC, **bad)


# ---- the statistics ---------------------------------------------------------------------------------------------------------
def test_null_statistics_by_hand():
    """C = 1, K = 2: category 0 (same = 0) holds the worked numbers, category 1 nothing at all"""
    obs = np.array([[5, 5], [0, 0]])
    expq = np.array([[3 * ONE, 3 * ONE], [0, 0]])                # x_0 = 2 for both states
    null_obs = np.zeros((4, 2, 2), dtype=np.int64)
    null_obs[:, 0, 0] = [4, 5, 5, 6]                             # x_t = 1, 2, 2, 3: two ties
    null_obs[:, 0, 1] = [3, 3, 3, 4]                             # x_t = 0, 0, 0, 1: all below
    null_expq = np.zeros((4, 2, 2), dtype=np.int64)
    null_expq[:, 0] = 3 * ONE
    st = enrich.null_statistics(obs, expq, null_obs, null_expq, 1)
    assert sorted(st) == sorted(enrich.STATISTICS) and all(st[k].shape == (1, 1, 2, 2) and st[k].dtype == np.float64 for k in st)
    get = lambda name: st[name][0, 0].tolist()
    assert get("null_mean") == [[2.0, 0.25], [0.0, 0.0]]
    assert np.allclose(st["null_sd"][0, 0], [[math.sqrt(2 / 3), 0.5], [0.0, 0.0]], rtol=1e-15)
    assert get("p_high") == [[0.8, 0.2], [1.0, 1.0]]             # ties count in both tails
    assert get("p_low") == [[0.8, 1.0], [1.0, 1.0]]
    assert get("p") == [[1.0, 0.4], [1.0, 1.0]]
    assert st["z"][0, 0, 0].tolist() == [0.0, 3.5] and np.isnan(st["z"][0, 0, 1]).all()      # sd = 0: no z, p = 1
    one = enrich.null_statistics(obs, expq, null_obs[:1], null_expq[:1], 1)                  # T = 1
    assert np.isnan(one["null_sd"]).all() and np.isnan(one["z"]).all()
    assert one["p_high"][0, 0].tolist() == [[0.5, 0.5], [1.0, 1.0]] and one["p_low"][0, 0].tolist() == [[1.0, 1.0], [1.0, 1.0]]
    # the comparison is made on the integers: an excess one unit of 2^-24 above x_0 is above it
    near = null_expq.copy()
    near[:, 0, 0] = null_obs[:, 0, 0] * ONE - (2 * ONE + 1)
    assert enrich.null_statistics(obs, expq, null_obs, near, 1)["p_low"][0, 0, 0, 0] == 0.2
    for bad in (dict(null_obs=null_obs[:, :1]), dict(null_obs=null_obs[:0], null_expq=null_expq[:0]), dict(obs=obs.astype(float))):
        with pytest.raises(ValueError):
            enrich.null_statistics(**dict(dict(obs=obs, expq=expq, null_obs=null_obs, null_expq=null_expq, C=1), **bad))


def test_null_statistics_fold_the_ordered_pairs():
    C, K, T = 2, 1, 3
    rng = np.random.default_rng(0)
    obs, null_obs = rng.integers(0, 9, (8, K)), rng.integers(0, 9, (T, 8, K))
    expq, null_expq = rng.integers(0, 9 * ONE, (8, K)), rng.integers(0, 9 * ONE, (T, 8, K))
    st = enrich.null_statistics(obs, expq, null_obs, null_expq, C)
    x = (null_obs * ONE - null_expq).reshape(T, C, C, 2, K)
    assert np.array_equal(st["null_mean"][0, 1], (x[:, 0, 1] + x[:, 1, 0]).astype(np.float64).mean(axis=0) / ONE)
    assert np.array_equal(st["null_mean"][1, 1], x[:, 1, 1].astype(np.float64).mean(axis=0) / ONE)
    assert not st["null_mean"][1, 0].any() and (st["p"][1, 0] == 1).all()


def test_null_lines_on_a_fixed_result():
    obs, expq = np.zeros((8, 2), dtype=np.int64), np.zeros((8, 2), dtype=np.int64)
    obs[2], obs[4], obs[7] = [3, 1], [1, 1], [0, 4]
    expq[2], expq[4], expq[7] = [2 * ONE, 2 * ONE], [ONE, ONE], [ONE, 3 * ONE]
    null_obs, null_expq = np.stack([obs, obs + 1, obs]), np.stack([expq, expq, expq])
    res = dict(obs=obs, expq=expq, K=2, C=2, **enrich.null_statistics(obs, expq, null_obs, null_expq, 2))
    lines = enrich.null_lines(res, ["none", "A"])
    assert lines[0] == enrich.NULL_HEADER + "\n" and lines[0].count("\t") == 11 and len(lines) == 5
    assert lines[1] == "none\tA\t0\t1\t4\t3.000\t1.667\t1.155\t-0.5774\t0.750000\t1.000000\t1.000000\n"      # x_t = 1, 3, 1 against x_0 = 1
    assert lines[4].startswith("A\tA\t1\t2\t4\t3.000\t1.333\t0.577\t")
    assert [ln.split("\t")[:5] for ln in lines[1:]] == [ln.split("\t")[:5] for ln in enrich.enrich_lines(
        dict(obs=obs, expected=expq / ONE, K=2, C=2), ["none", "A"])[1:]]


# ---- the constants ----------------------------------------------------------------------------------------------------------
def test_null_group_is_the_sources_rule():
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "enrich_null.hip")).read()
    for name in ("NULL_LDS_BYTES", "NULL_MAX_GROUP", "NULL_GRID_CAP", "NULL_CLASS_CAP", "NULL_CHUNK", "NULL_MAX_SHIFTS"):
        assert "%s = %d;" % (name, getattr(enrich, name)) in src, name
    tiles = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "enrich_tiles.h")).read()      # enrich.hip's tile, compiled here too
    assert "ENRICH_TILE_H = %d;" % enrich.TILE_H in tiles and "ENRICH_TILE_W = %d;" % enrich.TILE_W in tiles
    assert "NULL_BINS = ENRICH_TILE_H + ENRICH_TILE_W;" in src and "TILE_H =" not in src and "TILE_W =" not in src
    assert "const int per = 4 * 2 * C * C * K + 8 * NULL_BINS;" in src and "NULL_LDS_BYTES / per" in src
    assert enrich.null_group(64, 8) == 1 and enrich.null_group(20, 3) == 16 and enrich.null_group(1, 1) == 16
    assert enrich.null_group(64, 4) == 6 and enrich.null_group(20, 8) == 5 and enrich.null_group(64, 3) == 11
    for K in (1, 2, 20, 64):
        for C in (1, 2, 3, 8):
            ts = enrich.null_group(K, C)
            assert ts * (4 * 2 * C * C * K + 8 * (enrich.TILE_H + enrich.TILE_W)) <= 65536 and 1 <= ts <= 16
    assert '#include "enrich_tiles.h"' in src and '#include "runs.h"' in tiles and "enrich_null.hip" in open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "Makefile")).read()


def test_the_header_keeps_its_version_and_gains_one_entry_point():
    from phylo_hmrf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert "#define PHMRF_VERSION 127\n" in txt and _lib.ABI_VERSION == 127
    assert "PHMRF_API int phmrf_pair_enrichment_null(" in txt and "PHMRF_API int phmrf_pair_enrichment(" in txt
    assert len(_lib.SIGNATURES["phmrf_pair_enrichment_null"]) == 21 and len(_lib.SIGNATURES["phmrf_pair_enrichment"]) == 19


def test_check_null_size():
    enrich.check_null_size(1000, 20, 3)
    enrich.check_null_size(4096, 64, 8)
    enrich.check_null_size(8191, 64, 8)
    for n, K, C in ((8192, 64, 8), (10000, 64, 8), (0, 2, 2)):
        with pytest.raises(ValueError):
            enrich.check_null_size(n, K, C)


# ---- no GPU, no answer ------------------------------------------------------------------------------------------------------
def test_enrichment_null_needs_a_gpu(monkeypatch):
    from phylo_hmrf_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(RuntimeError) as e:
        enrich.enrichment_null(np.zeros(6857, dtype=np.int64), LEN_VEC, {1: np.zeros(10, dtype=np.uint8)}, n=3)
    assert "no CPU fallback" in str(e.value)


# ---- the command line -------------------------------------------------------------------------------------------------------
def _cli(output="unused", **extra):
    import phylo_hmrf as cli
    return cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", output, quiet="1", **extra)


ON = dict(enrich="a.mat", enrich_bed="a.bed")


@pytest.mark.parametrize("extra", [
    dict(enrich_null="10"),                                  # the three options without --enrich
    dict(enrich_null_min="5"),
    dict(enrich_null_seed="3"),
    dict(ON, enrich_null="-1"),
    dict(ON, enrich_null="10001"),
    dict(ON, enrich_null="many"),
    dict(ON, enrich_null="10", enrich_null_min="-5"),
    dict(ON, enrich_null="10", enrich_null_seed="-1"),
    dict(ON, enrich_null="10", enrich_null_min="1.5"),
    dict(ON, enrich_null_min="5"),                           # --enrich without --enrich_null N
    dict(ON, enrich_null_seed="3"),
])
def test_cli_refusals(extra):
    with pytest.raises(SystemExit) as e:
        _cli(**extra)
    assert "--enrich_null" in str(e.value)
    assert not os.path.exists("unused")


def test_cli_parses_the_options_with_their_defaults():
    import phylo_hmrf as cli
    o = cli.parse_args(["--enrich", "a.mat", "--enrich_bed", "a.bed"])
    assert (o.enrich_null, o.enrich_null_min, o.enrich_null_seed) == ("0", "1000000", "0")
    o = cli.parse_args(["--enrich", "a.mat", "--enrich_bed", "a.bed", "--enrich_null", "1000", "--enrich_null_min", "250000",
                        "--enrich_null_seed", "7"])
    assert (o.enrich_null, o.enrich_null_min, o.enrich_null_seed) == ("1000", "250000", "7")
    assert cli.check_enrich_null("", "0", "1000000", "0", "50000") == (0, 0, 0)
    assert cli.check_enrich_null("a.mat") == (0, 20, 0)
    assert cli.check_enrich_null("a.mat", "1000", "1000000", "0", "50000") == (1000, 20, 0)
    assert cli.check_enrich_null("a.mat", "10000", "10", "9", "50000") == (10000, 1, 9)          # at least one bin
    assert cli.check_enrich_null("a.mat", "1", "0", "0", "10000") == (1, 1, 0)


def _files(tmp_path, K, names):
    import scipy.io
    s = (np.arange(6857) % K).astype(np.int64)
    path = os.path.join(str(tmp_path), "estimate_ou_7.mat")
    scipy.io.savemat(path, dict(state_vec=s.reshape(1, -1), len_vec=LEN_VEC))
    bed = os.path.join(str(tmp_path), "a.bed")
    with open(bed, "w") as fh:
        fh.write("".join("chr1 %d %d %s\n" % (500000 * k, 500000 * k + 400000, names[k % len(names)]) for k in range(12)))
        fh.write("chr2 100000 2000000 %s\n" % names[0])
    return s, path, bed


def test_cli_refuses_tables_of_2_to_the_26_entries(tmp_path):
    """N 2 C C K is known once the map and the annotation are read; refused before any GPU work"""
    _, path, bed = _files(tmp_path, 64, ["n%d" % k for k in range(7)])
    out = os.path.join(str(tmp_path), "out")
    with pytest.raises(SystemExit) as e:
        _cli(output=out, enrich=path, enrich_bed=bed, enrich_null="10000")
    assert "--enrich_null" in str(e.value) and "2^26" in str(e.value) and not os.path.exists(out)


# ---- --enrich without --enrich_null is what it was --------------------------------------------------------------------------
KEYS = ["C", "K", "cat_dist", "class_1", "class_2", "class_5", "d0", "enrich_field", "expected", "len_vec", "log2_enrichment", "names",
        "obs", "obs_region", "resolution", "seg_1", "seg_2", "seg_5", "segments", "skipped_lines", "state_dist", "window", "window_bp"]


def _host_pair_enrichment(state_vec, len_vec, bin_class, bin_seg=None, window=(0, -1), K=None, C=None):
    """pair_enrichment's dict from the restatement: lets enrich_files run without a GPU"""
    s = np.asarray(state_vec).reshape(-1).astype(np.int64)
    K = int(s.max()) + 1 if K is None else K
    ref = R.pair_enrichment(s, len_vec, bin_class, bin_seg, window, K, C)
    exp = enrich.expected(ref["state_dist"], ref["cat_dist"])
    return dict(obs=ref["obs"], obs_region=ref["obs_region"], state_dist=ref["state_dist"], cat_dist=ref["cat_dist"],
                d0=np.int64(ref["d0"]), expected=exp, log2_enrichment=enrich.log2_enrichment(ref["obs"], exp),
                window=np.array(window, dtype=np.int64), K=np.int64(K), C=np.int64(C))


def test_enrich_without_the_null_writes_what_it_wrote(tmp_path, monkeypatch):
    """the same two files, the same arrays under the same names in the same order, the same text: every byte of the text and of
    every array (the .npz container itself carries the time of day)"""
    monkeypatch.setattr(enrich, "pair_enrichment", _host_pair_enrichment)
    s, path, bed = _files(tmp_path, 6, ["A", "B"])
    outs = []
    for name, extra in (("a", {}), ("b", dict(null=0, null_min_bp=5, null_seed=9))):
        out = enrich.enrich_files(path, bed, os.path.join(str(tmp_path), name), 50000, window_bp="100000-3000000", segments=True, **extra)
        assert sorted(os.listdir(os.path.dirname(out))) == ["enrich_estimate_ou_7.npz", "enrich_estimate_ou_7.txt"]
        outs.append(out)
    za, zb = (np.load(o, allow_pickle=False) for o in outs)
    first = ["len_vec", "resolution", "enrich_field", "window_bp", "segments", "names", "skipped_lines", "class_1", "class_2", "class_5",
             "seg_1", "seg_2", "seg_5", "obs", "obs_region", "state_dist", "cat_dist", "d0", "expected", "log2_enrichment", "window", "K", "C"]
    assert za.files == first == zb.files and sorted(za.files) == KEYS
    for k in za.files:
        assert za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes(), k
    ann = enrich.read_annotation(bed, LEN_VEC, 50000, segments=True)
    want = "".join(enrich.enrich_lines(_host_pair_enrichment(s, LEN_VEC, ann["bin_class"], ann["bin_seg"], (2, 60), None, 3), ann["names"]))
    for o in outs:
        assert open(o[:-4] + ".txt", "rb").read() == want.encode() and want.count("\n") > 10
