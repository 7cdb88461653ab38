"""CPU: the restatement of tests/regrid_reference.py pinned by hand and by identities, and the host parts of
phylo_hmrf_amd.regrid and of the command line's --regrid.  No GPU is touched: the GPU's results are held to the reference in
tests/test_gpu_regrid.py."""
import os
import re

import numpy as np
import pytest

from phylo_hmrf_amd import regrid
from tests import aggregate_reference, render_reference
from tests import regrid_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_A = [(7, 7, 0, 0, 1, 1), (12, 12, 7, 7, 1, 1), (7, 12, 0, 7, 0, 1)]      # two diagonal blocks and the block between them
LAYOUT_B = [(19, 19, 0, 0, 1, 1)]


# ---- the overlap ------------------------------------------------------------------------------------------------------------
def test_overlap_by_hand():
    hand = {
        (1, 5): {(0, 0): 1, (0, 4): 1, (0, 5): 0, (1, 5): 1, (1, 4): 0, (1, 9): 1, (1, 10): 0},
        (5, 1): {(0, 0): 1, (4, 0): 1, (5, 0): 0, (5, 1): 1, (9, 1): 1, (10, 1): 0, (10, 2): 1},
        (2, 5): {(0, 0): 2, (0, 1): 2, (0, 2): 1, (0, 3): 0, (1, 2): 1, (1, 3): 2, (1, 4): 2, (1, 5): 0, (2, 5): 2, (2, 7): 1},
        (5, 2): {(0, 0): 2, (1, 0): 2, (2, 0): 1, (2, 1): 1, (3, 1): 2, (3, 0): 0, (4, 1): 2, (5, 2): 2, (5, 1): 0},
        (3, 7): {(0, 0): 3, (0, 1): 3, (0, 2): 1, (0, 3): 0, (1, 2): 2, (1, 3): 3, (1, 4): 2, (1, 5): 0, (2, 4): 1, (2, 5): 3,
                 (2, 6): 3, (2, 7): 0},
    }
    for (a, b), cases in hand.items():
        for (x, p), want in cases.items():
            assert R.ov(x, p, a, b) == want, (a, b, x, p)
            assert regrid.overlap(x, p, a, b) == want, (a, b, x, p)
        for x in range(6):                                   # a target bin's overlaps sum to its b units
            assert sum(R.ov(x, p, a, b) for p in range(60)) == b
    assert regrid.overlap(3, 1 << 40, 7, 5) == 0
    assert regrid.ratio(10000, 50000) == (1, 5) and regrid.ratio(50000, 10000) == (5, 1) and regrid.ratio(20000, 50000) == (2, 5)
    assert regrid.ratio(1, 1 << 15) == (1, 1 << 15)
    for bad in ((1, (1 << 15) + 1), ((1 << 15) + 1, 1), (0, 5), (5, 0)):
        with pytest.raises(ValueError):
            regrid.ratio(*bad)
    assert [regrid.max_bins(a, b) for a, b in ((1, 5), (5, 1), (2, 5), (5, 2), (3, 7), (1, 40), (1, 1))] == [5, 1, 3, 2, 3, 40, 1]
    assert regrid.is_small(1, 16) and not regrid.is_small(1, 17) and regrid.is_small(5, 1)


def test_four_bins_by_hand():
    """One diagonal block of 4 bins halved (a = 1, b = 2).  Cell (0, 0) reads (0, 0) = 1, (1, 1) = 1 and (0, 1) = 0 twice: 2 votes
    each, the lowest state wins, and the off-diagonal source cell counted twice on a diagonal target cell.  Cell (0, 1) reads
    2, 2, 0, 3.  Cell (1, 1) reads (2, 2) = 3, (3, 3) = 3 and (2, 3) = 1 twice: state 1."""
    s = np.array([1, 0, 2, 2, 1, 0, 3, 3, 1, 3])
    L = R.len_vec_of([(4, 4, 0, 0, 1, 1)])
    D = R.len_vec_of([(2, 2, 0, 0, 1, 1)])
    got = R.regrid(s, L, D, 1, 2, 4, 1)
    assert got["state_vec"].tolist() == [0, 2, 1]
    assert got["support"].tolist() == [2, 2, 2] and got["covered"].tolist() == [4, 4, 4]
    assert got["hist_region"].tolist() == [[1, 1, 1, 0, 0]] and got["mixed_region"].tolist() == [3]
    C, bad = R.planes(s, L, 1, 4)
    assert R.cell_votes(C, bad, 1, 2, 0, 0).tolist() == [2, 2, 0, 0]
    assert R.cell_votes(C, bad, 1, 2, 0, 1).tolist() == [1, 0, 2, 1]
    assert R.cell_votes(C, bad, 1, 2, 1, 0).tolist() == [1, 0, 2, 1]         # the mirror half
    assert R.cell_votes(C, bad, 1, 2, 1, 1).tolist() == [0, 2, 0, 2]
    assert R.regrid(s, L, D, 1, 2, 4, 4)["state_vec"].tolist() == [0, 2, 1]  # covered == min_cover is called
    # the target one bin further on reads bins 2 .. 5, of which the map holds 2 and 3: the corner cell is a quarter covered
    D2 = R.len_vec_of([(2, 2, 1, 1, 1, 1)])
    got = R.regrid(s, L, D2, 1, 2, 4, 2)
    assert got["covered"].tolist() == [4, 0, 0] and got["state_vec"].tolist() == [1, 4, 4]
    assert got["hist_region"].tolist() == [[0, 1, 0, 0, 2]]
    # a state >= K counts only where it is read
    bad_s = s.copy()
    bad_s[0] = 9
    assert R.regrid(bad_s, L, D2, 1, 2, 4, 2)["state_vec"].tolist() == [1, 4, 4]
    with pytest.raises(ValueError):
        R.regrid(bad_s, L, D, 1, 2, 4, 1)


# ---- identities of the reference --------------------------------------------------------------------------------------------
def test_the_same_grid_gives_the_same_map():
    M = R.symmetric(19, 6, 1)
    L = R.len_vec_of(LAYOUT_A)
    s = R.state_vec_of(L, {1: M})
    got = R.regrid(s, L, L, 1, 1, 6, 1)
    assert np.array_equal(got["state_vec"], s)
    assert np.all(got["support"] == 1) and np.all(got["covered"] == 1) and not got["mixed_region"].any()


def test_a_to_b_to_a_across_two_splits():
    M = R.symmetric(19, 6, 2)
    LA, LB = R.len_vec_of(LAYOUT_A), R.len_vec_of(LAYOUT_B)
    sa = R.state_vec_of(LA, {1: M})
    sb = R.regrid(sa, LA, LB, 1, 1, 6, 1)["state_vec"]
    assert np.array_equal(sb, R.state_vec_of(LB, {1: M}))
    back = R.regrid(sb, LB, LA, 1, 1, 6, 1)
    assert np.array_equal(back["state_vec"], sa) and np.all(back["covered"] == 1)


@pytest.mark.parametrize("f", [2, 5])
def test_refining_then_coarsening_gives_the_map_back(f):
    M = R.symmetric(9, 5, 3)
    L = R.len_vec_of([(4, 4, 0, 0, 1, 1), (5, 5, 4, 4, 1, 1), (4, 5, 0, 4, 0, 1)])
    s = R.state_vec_of(L, {1: M})
    fine_L = R.len_vec_of([(9 * f, 9 * f, 0, 0, 1, 1)])
    fine = R.regrid(s, L, fine_L, f, 1, 5, 1)
    assert np.array_equal(fine["state_vec"], R.state_vec_of(fine_L, {1: np.kron(M, np.ones((f, f), dtype=np.int64))}))
    assert np.all(fine["covered"] == 1)
    back = R.regrid(fine["state_vec"], fine_L, L, 1, f, 5, f * f)
    assert np.array_equal(back["state_vec"], s)
    assert np.all(back["support"] == f * f) and np.all(back["covered"] == f * f)


@pytest.mark.parametrize("region", [(53, 53, 0, 0, 1, 1), (20, 33, 0, 25, 0, 1)])
def test_an_aligned_integer_factor_is_the_render_vote(region):
    f, K = 5, 4
    H, W, s1, s2, diag, _ = region
    L = R.len_vec_of([region])
    s = R.state_vec_of(L, {1: R.symmetric(60, K, 4, blocky=True)})
    h, w = -(-H // f), -(-W // f)
    D = R.len_vec_of([(h, w, s1 // f, s2 // f, diag, 1)])
    got = R.regrid(s, L, D, 1, f, K, 1)["state_vec"]
    want = render_reference.planes(s, H, W, diag, K, f)[0]
    assert np.array_equal(got, want[np.triu_indices(h)] if diag else want.reshape(-1))


def test_at_a_1_the_votes_are_aggregates_rectangle_counts():
    K, b = 5, 4
    L = R.len_vec_of(LAYOUT_A)
    s = R.state_vec_of(L, {1: R.symmetric(19, K, 5)})
    C, bad = R.planes(s, L, 1, K)
    for x, y in ((0, 0), (1, 1), (1, 2), (2, 1), (0, 4), (4, 4), (3, 1)):
        feature = [1, x * b, (x + 1) * b, y * b, (y + 1) * b, 0, 0]
        want = aggregate_reference.feature_hist(s, L, feature, 1, 0, K)[0, 0]
        assert np.array_equal(R.cell_votes(C, bad, 1, b, x, y), want), (x, y)


# ---- the host parts of the module -------------------------------------------------------------------------------------------
def test_derive_len_vec():
    L = R.len_vec_of([(7, 7, 0, 0, 1, 1), (12, 12, 7, 7, 1, 1), (7, 12, 0, 7, 0, 1), (10, 10, 3, 3, 1, 2)])
    L[:, 7] = [4, 5, 6, 9]
    D = regrid.derive_len_vec(L, 10000, 50000)
    assert D.tolist() == [[3, 0, 3, 2, 2, 0, 0, 4, 1, 1], [6, 3, 9, 3, 3, 1, 1, 5, 1, 1], [6, 9, 15, 2, 3, 0, 1, 6, 0, 1],
                          [6, 15, 21, 3, 3, 0, 0, 9, 1, 2]]
    D = regrid.derive_len_vec(L[:1], 50000, 10000)
    assert D.tolist() == [[35 * 36 // 2, 0, 35 * 36 // 2, 35, 35, 0, 0, 4, 1, 1]]
    D = regrid.derive_len_vec(L[1:3], 20000, 50000)          # bins [7, 19) of 2 units -> [14, 38) of 5: target bins 2 .. 7
    assert D[:, 3:7].tolist() == [[6, 6, 2, 2], [3, 6, 0, 2]]
    wide = np.concatenate([L, np.full((4, 2), 77)], axis=1)
    assert regrid.derive_len_vec(wide, 10000, 10000).tolist() == L.tolist()
    with pytest.raises(ValueError):
        regrid.derive_len_vec(L[:, :9], 10000, 50000)


def test_check_disjoint():
    regrid.check_disjoint(R.len_vec_of(LAYOUT_A))
    regrid.check_disjoint(R.len_vec_of([(7, 7, 0, 0, 1, 1), (7, 7, 0, 0, 1, 2)]))            # two chromosomes
    cases = [("rows 0 and 1 overlap", [(7, 7, 0, 0, 1, 1), (12, 12, 6, 6, 1, 1)]),
             ("rows 0 and 1 overlap", [(7, 7, 0, 0, 1, 1), (3, 5, 2, 5, 0, 1)]),                  # a block inside a diagonal block's square
             ("rows 1 and 2 overlap through the mirror", [(3, 3, 0, 0, 1, 1), (4, 5, 3, 10, 0, 1), (2, 2, 11, 5, 0, 1)]),
             ("row 1 overlaps its own mirror", [(3, 3, 0, 0, 1, 1), (5, 5, 4, 8, 0, 1)])]
    regrid.check_disjoint(R.len_vec_of([(7, 7, 0, 0, 1, 1), (5, 3, 7, 4, 0, 1)]))                # below the diagonal, beside the square
    for text, regions in cases:
        with pytest.raises(ValueError) as e:
            regrid.check_disjoint(R.len_vec_of(regions))
        assert text in str(e.value), (text, str(e.value))
    L = R.len_vec_of([(4, 4, 0, 1, 1, 1)])
    with pytest.raises(ValueError):
        regrid.check_disjoint(L)


def test_min_cover_and_the_k_64_refusal():
    assert regrid.min_cover_of(0, 5) == 1 and regrid.min_cover_of(50, 5) == 13 and regrid.min_cover_of(100, 5) == 25
    assert regrid.min_cover_of(48, 5) == 12 and regrid.min_cover_of("48.01", 5) == 13 and regrid.min_cover_of(4, 5) == 1
    assert regrid.min_cover_of(50, 1) == 1 and regrid.min_cover_of(100, 1 << 15) == 1 << 30
    assert regrid.min_cover_of(12.5, 4) == 2 and regrid.min_cover_of(np.int64(25), 2) == 1
    for bad in (-1, 101, "100.5"):
        with pytest.raises(ValueError):
            regrid.min_cover_of(bad, 5)
    regrid.check_uncalled(64, 0)
    regrid.check_uncalled(63, 10)
    with pytest.raises(ValueError):
        regrid.check_uncalled(64, 1)


def _result(s, L, D, a, b, K, min_cover):
    ref = R.regrid(s, L, D, a, b, K, min_cover)
    res = regrid.derived_planes(ref["state_vec"], ref["support"], ref["covered"], K, b)
    res.update(hist_region=ref["hist_region"], mixed_region=ref["mixed_region"], K=np.int64(K), fill=np.int64(K), a=np.int64(a),
               b=np.int64(b), min_cover=np.int64(min_cover))
    return res


def test_mat_round_trip_and_text(tmp_path):
    import scipy.io
    from phylo_hmrf_amd.maps import load_map
    K = 4
    L = R.len_vec_of([(13, 13, 0, 0, 1, 1)])
    s = R.state_vec_of(L, {1: R.symmetric(13, K, 6)})
    D = R.len_vec_of([(3, 3, 0, 0, 1, 1), (2, 2, 5, 5, 1, 2)])
    D = np.concatenate([D, np.full((2, 1), 7)], axis=1)      # a target's extra columns are kept
    res = _result(s, L, D, 1, 5, K, 13)
    assert res["conf"].dtype == np.float32 and res["cover"].dtype == np.float32
    called = res["state_vec"] != K
    assert np.array_equal(res["conf"][called], (res["support"][called] / res["covered"][called]).astype(np.float32))
    assert not res["conf"][~called].any() and np.array_equal(res["cover"], (res["covered"] / 25.0).astype(np.float32))
    path = str(tmp_path / "regrid_x_50000.mat")
    regrid.save_mat(path, res, D, L, 10000, 50000, cover=50, source="x.mat")
    state, len_vec, conf = load_map(path)
    assert np.array_equal(state, res["state_vec"]) and np.array_equal(len_vec, D) and np.array_equal(conf, res["conf"])
    d = scipy.io.loadmat(path)
    one = lambda name: int(np.asarray(d[name]).reshape(-1)[0])
    assert one("K") == K and one("uncovered_state") == K and one("regrid_from") == 10000 and one("resolution") == 50000
    assert np.array_equal(d["src_len_vec"], L) and np.array_equal(d["hist_region"], res["hist_region"])
    assert np.array_equal(d["support"].reshape(-1), res["support"]) and np.array_equal(d["covered"].reshape(-1), res["covered"])
    assert "fill" not in d
    lines = regrid.summary_lines(res, D)
    assert lines[0].startswith("#region\tchrom\t") and lines[0].rstrip("\n").endswith("state4\tuncovered") and len(lines) == 3
    f = lines[1].rstrip("\n").split("\t")
    hist = res["hist_region"][0]
    assert [int(x) for x in f[:8]] == [0, 1, 0, 0, 6, 6 - int(hist[K]), int(hist[K]), 6 - int(hist[K]) - int(res["mixed_region"][0])]
    assert f[8] == "%.6f" % res["cover"][:6].astype(np.float64).mean() and [int(x) for x in f[9:]] == hist.tolist()
    assert lines[2].split("\t")[4:8] == ["3", "0", "3", "0"]                # the chromosome the source lacks
    full = _result(s, L, D[:1], 1, 5, K, 1)
    regrid.save_mat(path, full, D[:1], L, 10000, 50000)
    assert int(scipy.io.loadmat(path)["uncovered_state"].reshape(-1)[0]) == -1


def test_without_a_gpu_it_raises():
    from phylo_hmrf_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = R.len_vec_of(LAYOUT_B)
    with pytest.raises(RuntimeError):
        regrid.regrid_states(np.zeros(190, dtype=np.int64), L, 10000, L, 50000)


# ---- the command line -------------------------------------------------------------------------------------------------------
REST = ("", "", "", "", "", "", "", "", "", "", "", "", "", "0", "0")       # segment .. filter_device
NAMES = ("segment", "postprocess", "compare", "domains", "render", "tracks", "enrich", "pileup", "consensus", "query", "aggregate",
         "ancestral", "save_model", "profile", "filter_device")


def test_check_regrid():
    import phylo_hmrf as cli
    assert cli.check_regrid("", "", "", "state_vec", "50", "50000", *REST) is None
    assert cli.check_regrid("m.mat", "10000", "", "state_vec", "50", "50000", *REST) == (10000, "50")
    assert cli.check_regrid("m.mat", "50000", "b.mat", "state_vec_smooth", "0", "10000", *REST) == (50000, "0")
    assert cli.check_regrid("m.mat", "20000", "", "state_vec", "12.5", "50000", *REST) == (20000, "12.5")
    for args in (("m.mat", "", "", "state_vec", "50"), ("m.mat", "x", "", "state_vec", "50"), ("m.mat", "0", "", "state_vec", "50"),
                 ("m.mat", "10000", "", "conf", "50"), ("m.mat", "10000", "", "state_vec", "101"),
                 ("m.mat", "10000", "", "state_vec", "-1"), ("m.mat", "10000", "", "state_vec", "half"),
                 ("m.mat", "1", "", "state_vec", "50"),                     # 1 : 50000 is above 2^15
                 # the sub-options without --regrid
                 ("", "10000", "", "state_vec", "50"), ("", "", "b.mat", "state_vec", "50"), ("", "", "", "state_vec_smooth", "50"),
                 ("", "", "", "state_vec", "40")):
        with pytest.raises(SystemExit):
            cli.check_regrid(*args, "50000", *REST)
    for at, name in enumerate(NAMES):
        other = list(REST)
        other[at] = "1" if name in ("profile", "filter_device") else "x.mat"
        with pytest.raises(SystemExit) as e:
            cli.check_regrid("m.mat", "10000", "", "state_vec", "50", "50000", *other)
        assert "--regrid cannot be combined with --%s" % name in str(e.value)
    opts = cli.parse_args(["--regrid", "m.mat", "--regrid_from", "10000", "--regrid_like", "b.mat"])
    assert (opts.regrid, opts.regrid_from, opts.regrid_like, opts.regrid_field, opts.regrid_cover) == ("m.mat", "10000", "b.mat",
                                                                                                      "state_vec", "50")


def test_every_other_mode_refuses_regrid():
    import phylo_hmrf as cli
    calls = {
        "ancestral": (cli.check_ancestral, ("posterior", "m.npz", "")),
        "profile": (cli.check_profile, ("1", "0.25,0.5", "", "")),
        "compare": (cli.check_compare, ("a.mat", "b.mat", "state_vec", "0", "", "", "", "", "0")),
        "domains": (cli.check_domains, ("a.mat", "state_vec", "", "", "", "", "", "0", "0")),
        "render": (cli.check_render, ("a.mat", "state_vec", "512", "0", "0", "", "", "", "", "", "", "0", "0")),
        "tracks": (cli.check_tracks, ("a.mat", "state_vec", "0-", "50000", "", "", "", "", "", "", "", "0", "0")),
        "enrich": (cli.check_enrich, ("a.mat", "a.bed", "state_vec", "0-", "0", "50000", "", "", "", "", "", "", "", "", "0", "0")),
        "pileup": (cli.check_pileup, ("a.mat", "a.bed", "", "state_vec", "100000", "0", "50000", "", "", "", "", "", "", "", "", "", "0", "0")),
        "consensus": (cli.check_consensus, ("a.mat,b.mat", "state_vec", "0", "-1", "-1", "", "", "", "", "", "", "", "", "", "", "0", "0")),
        "query": (cli.check_query, ("a.mat", "a.bed", "", "state_vec", "0", "50000", "", "", "", "", "", "", "", "", "", "", "", "0", "0")),
        "aggregate": (cli.check_aggregate, ("a.mat", "a.bed", "", "state_vec", "32", "16", "0", "0", "", "50000", "", "", "", "", "", "",
                                            "", "", "", "", "", "", "0", "0")),
    }
    for name, (check, args) in calls.items():
        check(*args)                                          # fine without --regrid, refused with it
        with pytest.raises(SystemExit) as e:
            check(*args, regrid="m.mat")
        assert "--regrid" in str(e.value), name


def test_the_command_line_refuses_before_any_gpu_use(monkeypatch):
    import phylo_hmrf as cli
    from phylo_hmrf_amd import maps

    def no_gpu():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(maps, "device", no_gpu)
    monkeypatch.setattr(regrid, "device", no_gpu)
    base = ["10", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1", "0.5", "8", "0",
            "0.001", "0", "1", "test", "0", "0", "60", "50000", "1", "hg38", "."]
    for extra in (dict(regrid="m.mat"), dict(regrid="m.mat", regrid_from="10000", compare="a.mat", compare_with="b.mat"),
                  dict(regrid="m.mat", regrid_from="10000", save_model="m.npz"), dict(regrid="m.mat", regrid_from="10000", profile="1"),
                  dict(regrid="m.mat", regrid_from="10000", filter_device="1"), dict(regrid="m.mat", regrid_from="10000", ancestral="called"),
                  dict(regrid_from="10000"), dict(regrid_cover="10"), dict(regrid="m.mat", regrid_from="10000", regrid_cover="200"),
                  dict(regrid="m.mat", regrid_from="10000", render="a.mat"), dict(regrid="m.mat", regrid_from="10000", aggregate="a.mat",
                                                                                   aggregate_bed="a.bed")):
        with pytest.raises(SystemExit):
            cli.run(*base, **extra)


def test_the_entry_point_is_declared():
    from phylo_hmrf_amd import _lib
    header = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert "#define PHMRF_VERSION 127\n" in header and _lib.ABI_VERSION == 127          # no ABI bump: an entry point only
    m = re.search(r"PHMRF_API int phmrf_regrid_states\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S)
    assert m and len(m.group(1).split(",")) == 20 == len(_lib.SIGNATURES["phmrf_regrid_states"])
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "regrid.hip")).read()
    for name, value in (("REGRID_LANES", regrid.LANES), ("REGRID_GRID_CAP", regrid.GRID_CAP), ("REGRID_SMALL_AREA", regrid.SMALL_AREA),
                        ("REGRID_WAVES", regrid.WAVES), ("REGRID_WAVE_GRID_CAP", regrid.WAVE_GRID_CAP),
                        ("REGRID_MAX_REGIONS", regrid.MAX_REGIONS), ("REGRID_ROW_W", regrid.ROW_W)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name
    assert "constexpr int REGRID_MAX_RATIO = 1 << 15;" in src and regrid.MAX_RATIO == 1 << 15
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", src))    # integers only
    assert "PHMRF_DETERMINISTIC" not in src and "asm" not in re.sub(r"//.*", "", src)
    assert "regrid.hip" in open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "Makefile")).read()
