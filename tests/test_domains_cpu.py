"""CPU: the yardstick of the domains of a state map (tests/domains_reference.py) on maps worked out by hand, the host side of
phylo_hmrf_amd.domains, and the command line's --domains refusals.  No GPU call is made here."""
import os

import numpy as np
import pytest

from phylo_hmrf_amd import domains
from tests import domains_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF, QUARTER = 1 << 23, 1 << 22          # floor(0.5 * 2^24), floor(0.25 * 2^24)

# A 4 x 4 diagonal block, upper triangle (nodes 0 - 9 row by row):      0 0 1 1
# state 0 runs along the diagonal (j - i <= 1: its own mirror),            0 0 1
# state 1 is the corner (j - i >= 2: it has a twin below the diagonal)       0 0
#                                                                              0
MAP_A = np.array([0, 0, 1, 1, 0, 0, 1, 0, 0, 0])
CONF_A = np.where(MAP_A == 0, 0.5, 0.25).astype(np.float32)
# cols:   root i0 i1 j0 j1 nodes area state boundary towards edges dmin dmax conf-sum 0 0
ROWS_A = [[0, 0, 3, 0, 3, 7, 10, 0, 7, 1, 7, 0, 1, 7 * HALF, 0, 0],
          [2, 0, 1, 2, 3, 3, 3, 1, 7, 0, 7, 2, 3, 3 * QUARTER, 0, 0]]

# A 5 x 3 full block with dist0 = 4 (nodes 3 i + j):      0 1 1     state 0 holds together through diagonal steps alone;
#                                                         2 0 1     state 1 has two components (roots 1 and 9);
#                                                         2 2 0     state 2 is one band of six nodes
#                                                         1 2 2
#                                                         1 1 2
MAP_B = np.array([0, 1, 1, 2, 0, 1, 2, 2, 0, 1, 2, 2, 1, 1, 2])
ROWS_B = [[0, 0, 2, 0, 2, 3, 3, 0, 12, 2, 7, 4, 4, 0, 0, 0],
          [1, 0, 1, 1, 2, 3, 3, 1, 7, 0, 5, 5, 6, 0, 0, 0],
          [3, 1, 4, 0, 2, 6, 6, 2, 16, 1, 9, 2, 3, 0, 0, 0],
          [9, 3, 4, 0, 1, 3, 3, 1, 7, 2, 7, 0, 1, 0, 0, 0]]


def test_diagonal_4x4_self_mirror_domain_and_twin_pair():
    got = D.region(MAP_A, 4, 4, True, 2, dist0=0, min_area=1, conf=CONF_A)
    assert got["table"].tolist() == ROWS_A
    assert got["n_components"].tolist() == [1, 1]
    assert got["domain_out"].tolist() == MAP_A.tolist()          # (domain 0 is state 0's, domain 1 state 1's)
    assert got["table"][:, 6].sum() + 3 == 16                    # the areas and the twin tile the full matrix
    adj = D.adjacency(MAP_A, 4, 4, True, 2)
    assert adj.tolist() == [[11, 7], [7, 3]]
    assert np.triu(adj).sum() == 21 == D.edges(4, 4, True)[0].size


def test_min_area_drops_rows_but_not_components():
    got = D.region(MAP_A, 4, 4, True, 2, min_area=4, conf=CONF_A)
    assert got["table"].tolist() == ROWS_A[:1]
    assert got["n_components"].tolist() == [1, 1]
    assert got["domain_out"].tolist() == np.where(MAP_A == 0, 0, -1).tolist()
    got = D.region(MAP_A, 4, 4, True, 2, min_area=11)
    assert got["table"].shape == (0, 16) and (got["domain_out"] == -1).all()


def test_full_5x3_diagonal_contact_and_two_components_of_one_state():
    got = D.region(MAP_B, 5, 3, False, 3, dist0=4)
    assert got["table"].tolist() == ROWS_B
    assert got["n_components"].tolist() == [1, 2, 1]
    assert got["domain_out"].tolist() == [0, 1, 1, 2, 0, 1, 2, 2, 0, 3, 2, 2, 3, 3, 2]
    adj = D.adjacency(MAP_B, 5, 3, False, 3)
    assert adj.tolist() == [[2, 5, 7], [5, 6, 9], [7, 9, 9]]
    assert np.triu(adj).sum() == 38 == D.edges(5, 3, False)[0].size


def test_neighbour_state_tie_takes_the_lowest_and_none_is_minus_one():
    got = D.region([1, 0, 2], 1, 3, False, 3, dist0=-1)
    assert got["table"].tolist() == [[0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0],
                                     [1, 0, 0, 1, 1, 1, 1, 0, 2, 1, 1, 0, 0, 0, 0, 0],
                                     [2, 0, 0, 2, 2, 1, 1, 2, 1, 0, 1, 1, 1, 0, 0, 0]]
    got = D.region([0, 0, 0], 2, 2, True, 1)
    assert got["table"].tolist() == [[0, 0, 1, 0, 1, 3, 4, 0, 0, -1, 0, 0, 1, 0, 0, 0]]
    assert D.adjacency([0, 0, 0], 2, 2, True, 1).tolist() == [[3]]


@pytest.mark.parametrize("H,W,diag,K,seed", [(4, 4, True, 2, 0), (5, 3, False, 3, 1), (9, 9, True, 4, 2), (7, 11, False, 5, 3),
                                              (1, 1, True, 1, 4), (1, 7, False, 2, 5)])
def test_edge_sums(H, W, diag, K, seed):
    """the adjacency's upper triangle holds every stored edge once; every discordant edge is a boundary edge of the two
    components it joins"""
    n = H * (H + 1) // 2 if diag else H * W
    s = np.random.default_rng(seed).integers(0, K, n)
    adj = D.adjacency(s, H, W, diag, K)
    assert np.array_equal(adj, adj.T)
    assert np.triu(adj).sum() == D.edges(H, W, diag)[0].size
    got = D.region(s, H, W, diag, K)
    assert got["all_boundary"] == got["table"][:, 8].sum() == 2 * np.triu(adj, 1).sum()
    assert got["table"][:, 5].sum() == n and got["n_components"].sum() == got["table"].shape[0]


def test_state_vec_domains_numbers_the_regions_and_summarises_the_states():
    lv = np.array([[10, 0, 10, 4, 4, 0, 0, 0, 1, 1], [15, 10, 25, 5, 3, 0, 4, 1, 0, 1]])
    sv = np.concatenate([MAP_A, MAP_B])
    ref = D.state_vec_domains(sv, lv, conf=np.concatenate([CONF_A, np.full(15, 1.0, dtype=np.float32)]), min_area=1)
    assert ref["domains"][:, 0].tolist() == [0, 0, 1, 1, 1, 1]
    assert ref["domains"][:2, 1:].tolist() == ROWS_A
    assert ref["domains"][2:, 1:14].tolist() == [r[:13] for r in ROWS_B]
    assert ref["domain_conf"].tolist() == [0.5, 0.25, 1.0, 1.0, 1.0, 1.0]
    assert ref["domain_vec"].tolist() == MAP_A.tolist() + [2, 3, 3, 4, 2, 3, 4, 4, 2, 5, 4, 4, 5, 5, 4]
    assert ref["components"].tolist() == [[1, 1, 0], [1, 2, 1]]
    assert ref["adjacency"].tolist() == [[13, 12, 7], [12, 9, 9], [7, 9, 9]]
    # nodes, components, listed domains, nodes in them, largest area, boundary edges
    assert ref["state_summary"].tolist() == [[10, 2, 2, 10, 10, 19], [9, 3, 3, 9, 3, 21], [6, 1, 1, 6, 6, 16]]
    assert domains.state_summary(ref["domains"], ref["adjacency"], ref["components"], np.bincount(sv)).tolist() == \
        ref["state_summary"].tolist()


def test_domain_lines_on_a_hand_made_table():
    lv = np.array([[18, 0, 18, 3, 6, 10, 20, 0, 0, 3]])
    table = np.array([[0, 9, 1, 2, 3, 5, 5, 7, 2, 9, 0, 4, 1, 4, 123, 0, 0],
                      [0, 0, 0, 0, 0, 0, 1, 1, 0, 0, -1, 0, 10, 10, 0, 0, 0]])
    lines = domains.domain_lines(table, np.array([0.75, np.nan]), lv, 50000)
    assert lines[0] == domains.HEADER and lines[0].count("\t") == 14
    assert lines[1] == "3\t550000\t650000\t3\t1150000\t1300000\t3\t7\t5\t0.750000\t9\t1\t4\t50000\t200000\n"
    assert lines[2] == "3\t500000\t550000\t3\t1000000\t1050000\t1\t1\t1\tnan\t0\t0\t0\t500000\t500000\n"
    assert "".join(lines) == D.lines(table, [0.75, np.nan], lv, 50000)


LV = np.array([[6, 0, 6, 3, 3, 0, 0, 0, 1, 1]])


def test_state_domains_refuses_bad_arguments_before_the_library():
    z = np.zeros(6, dtype=np.int64)
    with pytest.raises(ValueError):
        domains.state_domains(z[:5], LV)
    with pytest.raises(ValueError):
        domains.state_domains(z, LV, conf=np.ones(5))
    with pytest.raises(ValueError):
        domains.state_domains(z, LV, min_area=0)
    with pytest.raises(ValueError):
        domains.state_domains(z + 64, LV)
    with pytest.raises(ValueError):
        domains.state_domains(z + 0.5, LV)


def test_no_host_fallback():
    from phylo_hmrf_amd import _lib
    if _lib.device_count() == 0:                            # (tests/test_gpu_domains.py runs the call where there is one)
        with pytest.raises(RuntimeError):
            domains.state_domains(np.zeros(6, dtype=np.int64), LV)


def test_domains_files_refuses_a_file_without_the_field(tmp_path):
    import scipy.io
    path = str(tmp_path / "a.mat")
    scipy.io.savemat(path, dict(state_vec=np.zeros((1, 6), dtype=np.int64), len_vec=LV))
    with pytest.raises(ValueError, match="state_vec_smooth"):
        domains.domains_files(path, str(tmp_path), 50000, field="state_vec_smooth")
    with pytest.raises(ValueError, match="resolution"):
        domains.domains_files(path, str(tmp_path), 0)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("domains_")]


def _cli(**extra):
    import phylo_hmrf as cli
    return cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", "unused", quiet="1", **extra)


@pytest.mark.parametrize("extra", [
    dict(segment="m.npz"),
    dict(postprocess="x.mat"),
    dict(compare="a.mat", compare_with="b.mat"),
    dict(compare="a.mat"),
    dict(segment="m.npz", ancestral="posterior"),
    dict(ancestral="posterior"),
    dict(save_model="m.npz"),
    dict(profile="1"),
    dict(filter_device="1"),
    dict(domains_field="top"),
])
def test_cli_refusals(extra):
    with pytest.raises(SystemExit) as e:
        _cli(domains="a.mat", **extra)
    assert "--domains" in str(e.value)
    assert not os.path.exists("unused")


def test_cli_parses_the_options_with_their_defaults():
    import phylo_hmrf as cli
    o = cli.parse_args(["--domains", "a.mat"])
    assert (o.domains, o.domains_field, o.domains_area) == ("a.mat", "state_vec", "-1")
    o = cli.parse_args(["--domains", "a.mat", "--domains_field", "state_vec_smooth", "--domains_area", "4"])
    assert (o.domains_field, o.domains_area) == ("state_vec_smooth", "4")
    assert cli.parse_args([]).domains == ""


def test_constants_are_the_headers_and_the_sources():
    from phylo_hmrf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert "#define PHMRF_VERSION 127\n" in txt and _lib.ABI_VERSION == 127          # no ABI bump: entry points only
    assert "#define PHMRF_STATE_DOMAIN_COLS 16\n" in txt
    assert domains.STATE_DOMAIN_COLS == 16 == D.COLS
    for name in ("phmrf_state_adjacency", "phmrf_state_domains"):
        assert "PHMRF_API int %s(" % name in txt and name in _lib.SIGNATURES
        assert txt.count(name) >= 2                         # declared and described
    assert len(_lib.SIGNATURES["phmrf_state_adjacency"]) == 7 and len(_lib.SIGNATURES["phmrf_state_domains"]) == 14
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "domains.hip")).read()
    assert "DOM_GRID_CAP = %d;" % domains.GRID_CAP in src
    assert "domains.hip" in open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "Makefile")).read()
