"""CPU: the consensus' restatement (tests/consensus_reference.py) on maps worked by hand and on its identities, and the host
side of phylo_hmrf_amd.consensus: the renumbering tables, the .mat round trip, the text and the command line."""
import os

import numpy as np
import pytest

from phylo_hmrf_amd import consensus, maps
from tests import consensus_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _region(ms, K, H, W, diag=False, **kw):
    return R.consensus_region([np.asarray(m) for m in ms], K, H, W, diag, **kw)


# ---- the restatement by hand ------------------------------------------------------------------------------------------------
def test_one_map_is_its_own_consensus():
    a = [2, 0, 1, 1]
    r = _region([a], 3, 1, 4)
    assert r["consensus"].tolist() == a and r["support"].tolist() == [1, 1, 1, 1] and r["core"].tolist() == a
    assert r["support_hist"].tolist() == [[0, 1], [0, 2], [0, 1]]
    assert r["agree"].tolist() == [[[1, 0, 0], [0, 2, 0], [0, 0, 1]]] and r["pair"].tolist() == [[4]]


def test_two_maps_that_disagree_give_the_lower_state_with_support_one():
    r = _region([[3, 1, 2], [0, 1, 3]], 4, 1, 3)              # the majority of two maps is two
    assert r["consensus"].tolist() == [0, 1, 2] and r["support"].tolist() == [1, 2, 1]
    assert r["core"].tolist() == [4, 1, 4]                    # K = 4 stands for "unstable"
    assert r["pair"].tolist() == [[3, 1], [1, 3]]
    assert r["agree"][0][0].tolist() == [0, 0, 0, 1]          # where the consensus is 0, map 0 holds 3
    assert r["agree"][1][0].tolist() == [1, 0, 0, 0]
    assert r["support_hist"].tolist() == [[0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 0]]


def test_a_three_way_tie_goes_to_the_lowest_state():
    r = _region([[4, 2], [1, 2], [3, 0]], 5, 1, 2, min_support=1)
    assert r["consensus"].tolist() == [1, 2] and r["support"].tolist() == [1, 2] and r["core"].tolist() == [1, 2]
    r = _region([[4, 2], [1, 2], [3, 0]], 5, 1, 2)
    assert r["core"].tolist() == [5, 2]
    # a tie of two against two, with a fifth map elsewhere
    assert _region([[3], [1], [3], [1], [0]], 4, 1, 1)["consensus"].tolist() == [1]


def test_a_renumbering_that_is_not_injective_merges_states():
    ren = np.full((3, 64), 255, dtype=np.uint8)
    ren[0, :3] = [0, 1, 2]
    ren[1, :3] = [1, 1, 0]                                    # map 1's states 0 and 1 are both state 1
    ren[2, :4] = [2, 0, 255, 1]                               # map 2 has no state 2
    r = _region([[0, 1, 2], [0, 1, 2], [3, 3, 0]], 3, 1, 3, renumber=ren)
    # renumbered: [0 1 2], [1 1 0], [1 1 2]
    assert r["consensus"].tolist() == [1, 1, 2] and r["support"].tolist() == [2, 3, 2]
    assert r["pair"].tolist() == [[3, 1, 2], [1, 3, 2], [2, 2, 3]]
    with pytest.raises(AssertionError):
        _region([[0, 1, 2], [0, 1, 2], [3, 3, 2]], 3, 1, 3, renumber=ren)      # 255: not a state of map 2


def test_bands_of_a_diagonal_and_an_off_diagonal_block():
    # 3 x 3 diagonal: nodes (0,0) (0,1) (0,2) (1,1) (1,2) (2,2), d = 0 1 2 0 1 0 -> bands 0 1 2 0 1 0
    a = [0, 0, 1, 1, 1, 0]
    b = [0, 1, 1, 1, 0, 0]
    c = [0, 1, 0, 1, 0, 1]
    r = _region([a, b, c], 2, 3, 3, True)
    assert r["support"].tolist() == [3, 2, 2, 3, 2, 2]
    want = np.zeros((32, 3), dtype=np.int64)
    want[0], want[1], want[2] = [3, 3, 2], [2, 2, 0], [1, 1, 0]
    assert np.array_equal(r["bands"], want)
    r = _region([a, b, c], 2, 3, 3, True, min_support=3)
    want[0], want[1], want[2] = [3, 2, 2], [2, 0, 0], [1, 0, 0]
    assert np.array_equal(r["bands"], want)
    # 2 x 3 off-diagonal, dist0 = -2: d = |-2 + j - i| = 2 1 0 / 3 2 1 -> bands 2 1 0 / 2 2 1
    r = _region([a, b, c], 2, 2, 3, False, dist0=-2)
    want = np.zeros((32, 3), dtype=np.int64)
    want[0], want[1], want[2] = [1, 1, 0], [2, 2, 0], [3, 3, 2]
    assert np.array_equal(r["bands"], want)
    r = _region([a, b, c], 2, 2, 3, False, dist0=5)           # d = 5 6 7 / 4 5 6: all in band 3
    assert r["bands"][3].tolist() == [6, 6, 2] and r["bands"].sum() == 14


@pytest.mark.parametrize("M,K,H,W,diag", [(1, 3, 7, 7, True), (2, 5, 6, 9, False), (5, 4, 11, 11, True), (16, 64, 9, 5, False)])
def test_identities_of_the_tables(M, K, H, W, diag):
    rng = np.random.default_rng(M * 100 + K)
    n = H * (H + 1) // 2 if diag else H * W
    ms = [rng.integers(0, K, n) for _ in range(M)]
    for min_support in (1, M // 2 + 1, M):
        r = _region(ms, K, H, W, diag, dist0=3, min_support=min_support)
        hist, agree, pair, bands = r["support_hist"], r["agree"], r["pair"], r["bands"]
        assert hist.sum() == n and not hist[:, 0].any()
        for m in range(M):
            assert np.array_equal(agree[m].sum(axis=1), hist.sum(axis=1))
            assert pair[m][m] == n
        assert sum(np.trace(agree[m]) for m in range(M)) == (hist * np.arange(M + 1)).sum()
        assert np.array_equal(pair, pair.T)
        assert bands[:, 0].sum() == n
        assert bands[:, 1].sum() == hist[:, min_support:].sum() == (r["core"] < K).sum()
        assert bands[:, 2].sum() == hist[:, M].sum()


# ---- the host side of the module --------------------------------------------------------------------------------------------
def test_majority_support_and_map_checks():
    assert [consensus.majority(M) for M in (1, 2, 3, 4, 5, 16)] == [1, 2, 2, 3, 3, 9]
    assert consensus.check_support(None, 5) == 3 and consensus.check_support(5, 5) == 5 and consensus.check_support(1, 1) == 1
    for bad in (0, 6, -1):
        with pytest.raises(ValueError, match="outside"):
            consensus.check_support(bad, 5)
    assert consensus.check_maps([[0, 1], [1, 1]]).tolist() == [[0, 1], [1, 1]]
    with pytest.raises(ValueError, match="nodes"):
        consensus.check_maps([[0, 1], [1, 1, 1]])
    with pytest.raises(ValueError, match="1 .. 16"):
        consensus.check_maps([[0]] * 17)
    with pytest.raises(ValueError, match="1 .. 16"):
        consensus.check_maps([])
    with pytest.raises(ValueError):
        consensus.check_maps([[0, 64]])


def test_renumbering_tables():
    t = consensus.identity_table(2, 3)
    assert t.shape == (2, 64) and t.dtype == np.uint8 and t[1, :4].tolist() == [0, 1, 2, 255] and (t[:, 3:] == 255).all()
    # map 1 is map 0 under the permutation 0 -> 2, 1 -> 0, 2 -> 1; map 2 has one state more than map 0
    C1 = np.array([[0, 0, 9], [7, 0, 0], [0, 8, 0]])
    C2 = np.array([[5, 0, 0, 1], [0, 0, 6, 0], [0, 4, 0, 2]])
    t = consensus.matched_table([C1, C2], 3)
    assert t[0, :4].tolist() == [0, 1, 2, 255]
    assert t[1, :4].tolist() == [1, 2, 0, 255]
    assert t[2, :5].tolist() == [0, 2, 1, 3, 255]
    # the left-over states of two maps are not merged
    t = consensus.matched_table([C2, C2], 3)
    assert t[1, :4].tolist() == [0, 2, 1, 3] and t[2, :4].tolist() == [0, 2, 1, 4]
    with pytest.raises(ValueError, match="64"):
        consensus.matched_table([np.eye(40, 60, dtype=np.int64)] * 2, 40)


def _two_regions():
    """a diagonal block of 4 bins and the 4 x 3 block beside it, three maps at K = 3"""
    rng = np.random.default_rng(5)
    n1, n2 = 10, 12
    L = np.array([[n1, 0, n1, 4, 4, 0, 0, 0, 1, 1], [n2, n1, n1 + n2, 4, 3, 0, 6, 1, 0, 1]], dtype=np.int64)
    truth = rng.integers(0, 3, n1 + n2)
    ms = []
    for _ in range(3):
        m = truth.copy()
        hit = rng.random(m.size) < 0.3
        m[hit] = rng.integers(0, 3, int(hit.sum()))
        ms.append(m)
    return ms, L


def test_reference_of_a_state_vec_adds_the_regions_up():
    ms, L = _two_regions()
    res = R.consensus_state_vec(ms, L, 3)
    a = R.consensus_region([m[:10] for m in ms], 3, 4, 4, True, 0, 2)
    b = R.consensus_region([m[10:] for m in ms], 3, 4, 3, False, 6, 2)
    assert np.array_equal(res["state_vec"], np.concatenate([a["consensus"], b["consensus"]]))
    assert np.array_equal(res["support_hist"], a["support_hist"] + b["support_hist"])
    assert np.array_equal(res["band_counts"], np.stack([a["bands"], b["bands"]]))
    assert res["conf"].dtype == np.float32 and np.array_equal(res["conf"], res["support"] / np.float32(3))
    assert res["pair_agreement"][1][1] == 1.0 and res["min_support"] == 2 and res["M"] == 3


def test_mat_round_trip_through_load_map(tmp_path):
    import scipy.io
    ms, L = _two_regions()
    res = R.consensus_state_vec(ms, L, 3)
    res.update(consensus.map_scores(res["agree"]))
    out = str(tmp_path / "consensus_a_3.mat")
    consensus.save_mat(out, res, L, ["a.mat", "b.mat", "c.mat"], 50000, "state_vec", True, None)
    s, L2, conf = maps.load_map(out)
    assert np.array_equal(s, res["state_vec"]) and np.array_equal(L2, L)
    assert conf.dtype == np.float32 and np.array_equal(conf, res["conf"])
    core, _, _ = maps.load_map(out, "core_vec")
    assert np.array_equal(core, res["core_vec"]) and core.max() <= 3
    d = scipy.io.loadmat(out)
    for k in ("support_hist", "support_hist_region", "agree", "pair", "band_counts", "renumber"):
        assert np.array_equal(d[k], res[k]), k
    assert np.allclose(d["pair_agreement"], res["pair_agreement"]) and d["agreement"].size == 3
    assert [d[k].item() for k in ("K", "M", "min_support", "consensus_match", "resolution")] == [3, 3, 2, 1, 50000]
    assert d["consensus_area"].reshape(-1).tolist() == [26, 26]
    assert [str(x[0]) for x in d["consensus_files"].reshape(-1)] == ["a.mat", "b.mat", "c.mat"]
    # K = 64: no core plane, and the file says so by not holding one
    res64 = dict(res, core_vec=None)
    consensus.save_mat(out, res64, L, ["a.mat", "b.mat", "c.mat"], 50000)
    assert "core_vec" not in scipy.io.loadmat(out)


def test_summary_lines():
    ms, L = _two_regions()
    res = R.consensus_state_vec(ms, L, 4)                     # state 4 never occurs
    res.update(consensus.map_scores(res["agree"]))
    lines = consensus.summary_lines(res, ["a.mat", "b.mat", "c.mat"])
    assert lines[0] == "#map\tpath\tagreement\tari\tnmi\tmean_pair_agreement\n"
    assert lines[4] == "#state\tnodes\tmean_support\tunanimous\tstable\n" and len(lines) == 9
    f = lines[2].rstrip("\n").split("\t")
    assert f[:2] == ["2", "b.mat"]
    assert float(f[2]) == pytest.approx(np.mean(ms[1] == res["state_vec"]), abs=1e-6)
    assert float(f[5]) == pytest.approx((np.mean(ms[1] == ms[0]) + np.mean(ms[1] == ms[2])) / 2, abs=1e-6)
    hist = res["support_hist"]
    f = lines[5].rstrip("\n").split("\t")
    assert int(f[0]) == 1 and int(f[1]) == hist[0].sum()
    assert float(f[2]) == pytest.approx(res["support"][res["state_vec"] == 0].mean(), abs=1e-6)
    assert float(f[3]) == pytest.approx(hist[0, 3] / hist[0].sum(), abs=1e-6)
    assert float(f[4]) == pytest.approx(hist[0, 2:].sum() / hist[0].sum(), abs=1e-6)
    assert lines[8] == "4\t0\t0.000000\t0.000000\t0.000000\n"
    one = R.consensus_state_vec(ms[:1], L, 3)
    one.update(consensus.map_scores(one["agree"]))
    assert consensus.summary_lines(one, ["a.mat"])[1] == "1\ta.mat\t1.000000\t1.000000\t1.000000\t1.000000\n"


def _write(tmp_path, name, s, L, **extra):
    import scipy.io
    p = str(tmp_path / name)
    scipy.io.savemat(p, dict(dict(state_vec=s, len_vec=L), **extra))
    return p


def test_consensus_files_refuses_before_it_needs_a_gpu(tmp_path):
    ms, L = _two_regions()
    a, b, c = (_write(tmp_path, "%s.mat" % x, m, L) for x, m in zip("abc", ms))
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="2 .. 16 files"):
        consensus.consensus_files([a], out, 50000)
    with pytest.raises(ValueError, match="2 .. 16 files"):
        consensus.consensus_files([a] * 17, out, 50000)
    L2 = L.copy()
    L2[1, 6] = 7                                              # another start bin
    other = _write(tmp_path, "other.mat", ms[1], L2)
    with pytest.raises(ValueError) as e:
        consensus.consensus_files([a, b, other], out, 50000)
    assert a in str(e.value) and other in str(e.value) and "len_vec" in str(e.value)
    one_region = _write(tmp_path, "one.mat", ms[1][:10], L[:1])
    with pytest.raises(ValueError, match="same regions"):
        consensus.consensus_files([a, one_region], out, 50000)
    with pytest.raises(ValueError, match="field"):
        consensus.consensus_files([a, b], out, 50000, field="conf")
    with pytest.raises(ValueError, match="state_vec_smooth"):
        consensus.consensus_files([a, b], out, 50000, field="state_vec_smooth")      # a field the files do not hold
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="outside"):
            consensus.consensus_files([a, b, c], out, 50000, min_support=bad)
    with pytest.raises(ValueError, match="resolution"):
        consensus.consensus_files([a, b], out, 0)
    with pytest.raises(ValueError, match="min_area"):
        consensus.consensus_files([a, b], out, 50000, min_area=0)
    assert not os.path.exists(out)


def test_consensus_states_has_no_host_fallback():
    from phylo_hmrf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or _lib.device_count() > 0:
        pytest.skip("needs the library and no GPU")
    ms, L = _two_regions()
    with pytest.raises(RuntimeError):
        consensus.consensus_states(ms, L)


# ---- the command line -------------------------------------------------------------------------------------------------------
QUIET = ("", "", "", "", "", "", "", "", "", "", "0", "0")


def test_cli_parses_the_options_with_their_defaults():
    import phylo_hmrf as cli
    o = cli.parse_args(["--consensus", "a.mat,b.mat"])
    assert (o.consensus, o.consensus_field, o.consensus_match, o.consensus_support, o.consensus_area) == \
        ("a.mat,b.mat", "state_vec", "0", "-1", "-1")
    o = cli.parse_args(["--consensus", "a.mat,b.mat,c.mat", "--consensus_field", "state_vec_smooth", "--consensus_match", "1",
                        "--consensus_support", "3", "--consensus_area", "40"])
    assert (o.consensus_field, o.consensus_match, o.consensus_support, o.consensus_area) == ("state_vec_smooth", "1", "3", "40")
    assert cli.parse_args([]).consensus == ""
    off = ("top", "x", "y", "z", "s.npz", "p.mat", "c.mat", "d.mat", "r.mat", "t.mat", "e.mat", "u.mat", "posterior", "m.npz", "1", "1")
    assert cli.check_consensus("", *off) is None              # off: nothing to refuse
    assert cli.check_consensus("a.mat,b.mat", "state_vec", "0", "-1", "-1", *QUIET) == (["a.mat", "b.mat"], None, None)
    assert cli.check_consensus("a.mat,b.mat,c.mat", "state_vec_smooth", "1", "3", "40", *QUIET) == \
        (["a.mat", "b.mat", "c.mat"], 3, 40)


def test_cli_refusals():
    import phylo_hmrf as cli
    ok = ("state_vec", "0", "-1", "-1")
    for files in ("a.mat", "a.mat,", ",".join(["a.mat"] * 17)):
        with pytest.raises(SystemExit, match="2 .. 16"):
            cli.check_consensus(files, *ok, *QUIET)
    with pytest.raises(SystemExit, match="--consensus_field"):
        cli.check_consensus("a.mat,b.mat", "conf", "0", "-1", "-1", *QUIET)
    with pytest.raises(SystemExit, match="--consensus_match"):
        cli.check_consensus("a.mat,b.mat", "state_vec", "2", "-1", "-1", *QUIET)
    for support in ("0", "3", "-2", "x"):
        with pytest.raises(SystemExit, match="--consensus_support"):
            cli.check_consensus("a.mat,b.mat", "state_vec", "0", support, "-1", *QUIET)
    for area in ("0", "-5"):
        with pytest.raises(SystemExit, match="--consensus_area"):
            cli.check_consensus("a.mat,b.mat", "state_vec", "0", "-1", area, *QUIET)
    names = ("--segment", "--postprocess", "--compare", "--domains", "--render", "--tracks", "--enrich", "--pileup", "--ancestral",
             "--save_model", "--profile 1", "--filter_device 1")
    for k, name in enumerate(names):
        other = list(QUIET)
        other[k] = "1" if k >= 10 else "x"
        with pytest.raises(SystemExit) as e:
            cli.check_consensus("a.mat,b.mat", *ok, *other)
        assert "--consensus cannot be combined with %s" % name in str(e.value)


def test_every_other_mode_refuses_consensus():
    import phylo_hmrf as cli
    both = "a.mat,b.mat"
    calls = {
        "--pileup": lambda: cli.check_pileup("a.mat", "a.bed", "", "state_vec", "1000000", "0", "50000", *QUIET[:9], "0", "0",
                                             consensus=both),
        "--enrich": lambda: cli.check_enrich("a.mat", "a.bed", "state_vec", "0-", "0", "50000", *QUIET[:8], "0", "0", consensus=both),
        "--tracks": lambda: cli.check_tracks("a.mat", "state_vec", "0-", "50000", *QUIET[:7], "0", "0", consensus=both),
        "--render": lambda: cli.check_render("a.mat", "state_vec", "64", "0", "0", *QUIET[:6], "0", "0", consensus=both),
        "--domains": lambda: cli.check_domains("a.mat", "state_vec", *QUIET[:5], "0", "0", consensus=both),
        "--compare": lambda: cli.check_compare("a.mat", "b.mat", "state_vec", "0", *QUIET[:4], "0", consensus=both),
        "--profile 1": lambda: cli.check_profile("1", "0.5", "", "", consensus=both),
    }
    for name, call in calls.items():
        with pytest.raises(SystemExit) as e:
            call()
        assert "%s cannot be combined with --consensus" % name in str(e.value), name


def test_cli_run_refuses_a_second_mode_before_anything_is_read(tmp_path):
    import phylo_hmrf as cli
    o = cli.parse_args(["--consensus", "a.mat,b.mat", "--domains", "a.mat", "--output", str(tmp_path / "unused")])
    with pytest.raises(SystemExit, match="--consensus cannot be combined with --domains"):
        cli.run(o.num_states, o.chromvec, o.root_path, o.multiple, o.species_name, o.sort_states, o.run_id, o.cons_param,
                o.method_mode, o.initial_mode, o.initial_weight, o.initial_weight1, o.initial_magnitude, o.position1, o.position2,
                o.filter_sigma, o.beta, o.beta1, o.num_neighbor, o.filter_mode, o.threshold, o.estimate_type, o.simu_version,
                o.annotation, o.reload, o.dtype, o.miter, o.resolution, o.quantile, o.ref_species, o.output, domains=o.domains,
                consensus=o.consensus)
    assert not os.path.exists(str(tmp_path / "unused"))


def test_constants_are_the_headers_and_the_sources():
    from phylo_hmrf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert "#define PHMRF_VERSION 127\n" in txt and _lib.ABI_VERSION == 127          # no ABI bump: an entry point only
    assert "#define PHMRF_CONSENSUS_MAPS %d\n" % consensus.CONSENSUS_MAPS in txt
    assert "PHMRF_API int phmrf_label_consensus(" in txt
    assert len(_lib.SIGNATURES["phmrf_label_consensus"]) == 17
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "consensus.hip")).read()
    assert "CONS_GRID_CAP = %d;" % consensus.CONSENSUS_GRID_CAP in src
    assert "CONS_PER_TRIP = %d;" % consensus.CONSENSUS_PER_TRIP in src
    assert "CONS_AGREE_BINS = %d;" % consensus.CONSENSUS_AGREE_BINS in src
    assert '#include "runs.h"' in src and "getenv" not in src and "asm" not in src
    assert "float" not in src and "double" not in src
    assert "consensus.hip" in open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "Makefile")).read()
    assert consensus.NOT_A_STATE == R.NOT_A_STATE == 255
