"""CPU: the comparison of two state maps.  The full-matrix restatement (tests/compare_reference.py, the yardstick of the GPU
calls) on hand-worked maps, the scores and the state matching of phylo_hmrf_amd.compare on tables with known answers, the
refusals of compare_files and of the command line ahead of any library call, and the header."""
import os

import numpy as np
import pytest
import scipy.io

from phylo_hmrf_amd import compare
from tests import compare_reference as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _upper(M):
    M = np.asarray(M)
    return M[np.triu_indices(M.shape[0])]


# ---- the restatement on hand-worked maps ---------------------------------------------------------------------------------
def test_contingency_counts_stored_nodes():
    a = np.array([0, 0, 1, 1, 1, 2])
    b = np.array([1, 0, 1, 1, 0, 0])
    assert C.contingency(a, b, 3, 2).tolist() == [[1, 1], [1, 2], [1, 0]]
    assert C.contingency(a, a, 3, 3).tolist() == [[2, 0, 0], [0, 3, 0], [0, 0, 1]]


def test_diff_codes_with_a_map_and_confidences_on_both_sides_of_the_threshold():
    a = np.array([0, 1, 1, 0, 2])
    b = np.array([1, 0, 1, 0, 2])
    assert C.diff_codes(a, b).tolist() == [2, 2, 0, 0, 0]
    assert C.diff_codes(a, b, map_b=[1, 0, 2]).tolist() == [0, 0, 2, 2, 0]
    ca = np.array([0.9, 0.5, 0.4, 0.9, 0.1], dtype=np.float32)
    cb = np.array([0.5, 0.49999, 0.9, 0.9, 0.9], dtype=np.float32)
    assert C.diff_codes(a, b, None, ca, cb, 0.5).tolist() == [2, 1, 0, 0, 0]       # 0.5 >= 0.5 counts, 0.49999 does not
    assert C.diff_codes(a, b, None, ca, cb, 0.0).tolist() == [2, 2, 0, 0, 0]       # min_conf 0: every difference counts


def test_self_mirror_domain_of_a_3x3_diagonal_block():
    A = np.zeros((3, 3), dtype=np.int64)
    B = A.copy()
    B[0, 0] = B[0, 1] = B[1, 0] = 1      # stored nodes (0,0) (0,1); full-matrix pixels (0,0) (0,1) (1,0): area 2 * 2 - 1 = 3
    diff, table, bands = C.compare_region(_upper(A), _upper(B), 3, 3, True)
    assert diff.tolist() == [2, 2, 0, 0, 0, 0]
    assert table.tolist() == [[0, 0, 0, 0, 1, 2, 3, 0, 1, 0, 0, 0]]
    assert bands[:3].tolist() == [[3, 1, 1], [2, 1, 1], [1, 0, 0]] and not bands[3:].any()
    assert C.compare_region(_upper(A), _upper(B), 3, 3, True, min_area=3)[1].shape == (1, 12)
    assert C.compare_region(_upper(A), _upper(B), 3, 3, True, min_area=4)[1].shape == (0, 12)


def test_twin_domain_of_a_4x4_diagonal_block_is_listed_once():
    A = np.zeros((4, 4), dtype=np.int64)
    B = A.copy()
    B[0, 3] = B[3, 0] = 2                # (0,3) and its mirror (3,0) do not touch: two components of area 1, one listed
    _, table, _ = C.compare_region(_upper(A), _upper(B), 4, 4, True)
    assert table.tolist() == [[3, 0, 0, 3, 3, 1, 1, 0, 2, 0, 0, 0]]
    B = A.copy()
    B[0, 2] = B[2, 0] = 2                # j - i == 2: still twins (the pixels are two apart)
    _, table, _ = C.compare_region(_upper(A), _upper(B), 4, 4, True)
    assert table.tolist() == [[2, 0, 0, 2, 2, 1, 1, 0, 2, 0, 0, 0]]


def test_domain_touching_the_diagonal_at_distance_one_is_its_own_mirror():
    A = np.zeros((4, 4), dtype=np.int64)
    B = A.copy()
    B[1, 2] = B[2, 1] = 1                # (1,2) and (2,1) touch at a corner: one component, area 2 * 1 - 0 = 2, one stored node
    _, table, _ = C.compare_region(_upper(A), _upper(B), 4, 4, True)
    assert table.tolist() == [[5, 1, 1, 2, 2, 1, 2, 0, 1, 0, 0, 0]]
    assert C.compare_region(_upper(A), _upper(B), 4, 4, True, min_area=3)[1].shape == (0, 12)


def test_modes_take_the_lowest_state_on_ties_and_the_sums_are_fixed_point():
    a = np.array([3, 1, 1, 3, 0, 0])     # 2 x 3 off-diagonal block
    b = np.array([2, 2, 0, 0, 0, 0])     # differs at nodes 0 - 3, one domain; A: 3 twice, 1 twice -> 1; B: 2 twice, 0 twice -> 0
    ca = np.array([0.5, 0.1, 1.0, 0.0, 0.3, 0.3], dtype=np.float32)
    cb = np.ones(6, dtype=np.float32)
    diff, table, bands = C.compare_region(a, b, 2, 3, False, dist0=1, conf_a=ca, conf_b=cb)
    assert diff.tolist() == [2, 2, 2, 2, 0, 0]
    assert table.tolist() == [[0, 0, 1, 0, 2, 4, 4, 1, 0, (1 << 23) + 1677721 + (1 << 24), 4 << 24, 0]]
    # d = |1 + j - i|: row 0 -> 1 2 3, row 1 -> 0 1 2
    assert bands[:3].tolist() == [[1, 1, 1], [2, 1, 1], [3, 2, 2]]
    # B renumbered 0 -> 3, 2 -> 1: b' = 1 1 3 3 3 3, nodes 1 and 3 now agree; (0,0) (0,2) (1,1) (1,2) touch at corners: one
    # domain, A's states 3 1 0 0 -> 0, B's 1 3 3 3 -> 3
    _, table, _ = C.compare_region(a, b, 2, 3, False, map_b=[3, 0, 1])
    assert table[:, [0, 1, 2, 3, 4, 5, 6, 7, 8]].tolist() == [[0, 0, 1, 0, 2, 4, 4, 0, 3]]


def test_band_edges():
    assert C.band_of([0, 1, 2, 3, 4, 7, 8, 2 ** 30, 2 ** 31 - 1]).tolist() == [0, 1, 2, 2, 3, 3, 4, 31, 31]


def test_compare_state_vec_numbers_the_regions():
    a = np.zeros(6 + 6, dtype=np.int64)
    b = a.copy()
    b[0] = 1
    b[6 + 5] = 1
    lv = np.array([[6, 0, 6, 3, 3, 0, 0, 0, 1, 1], [6, 6, 12, 2, 3, 0, 10, 1, 0, 1]])
    diff, table, bands = C.compare_state_vec(a, b, lv, min_area=1)
    assert table[:, :2].tolist() == [[0, 0], [1, 5]] and diff.sum() == 4 and bands.shape == (2, 32, 3)
    assert bands[1, :, 0].sum() == 6 and bands[1, 4, 0] == 6          # d = 10 + j - i in 9 .. 12: band 4 (8 - 15)
    assert C.compare_state_vec(a, b, lv)[1].shape == (0, 13)          # the default area rule: 26 for so small a region


# ---- scores and matching ---------------------------------------------------------------------------------------------------
def _table(a, b):
    return C.contingency(a, b, int(a.max()) + 1, int(b.max()) + 1)


def test_scores_of_identical_maps():
    a = np.random.default_rng(0).integers(0, 5, 1000)
    s = compare.scores(_table(a, a))
    assert s["agreement"] == 1.0 and s["ari"] == pytest.approx(1.0, abs=1e-12) and s["nmi"] == pytest.approx(1.0, abs=1e-12)


def test_scores_of_a_permutation_before_and_after_matching():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 6, 5000)
    perm = np.array([3, 0, 5, 1, 2, 4])
    b = perm[a]
    T = _table(a, b)
    s = compare.scores(T)
    assert s["agreement"] == 0.0 and s["ari"] == pytest.approx(1.0, abs=1e-12) and s["nmi"] == pytest.approx(1.0, abs=1e-12)
    map_b = compare.match_states(T)
    assert map_b.dtype == np.uint8 and np.array_equal(map_b, np.argsort(perm))      # the inverse permutation
    assert np.array_equal(map_b[b], a)
    s = compare.scores(compare.permute_columns(T, map_b))
    assert s["agreement"] == 1.0 and s["ari"] == pytest.approx(1.0, abs=1e-12)


def test_scores_of_independent_and_single_cluster_maps():
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 4, 200000), rng.integers(0, 4, 200000)
    s = compare.scores(_table(a, b))
    assert abs(s["ari"]) < 1e-3 and 0 <= s["nmi"] < 1e-3 and abs(s["agreement"] - 0.25) < 0.01
    z = np.zeros(50, dtype=np.int64)
    assert compare.scores(_table(z, z)) == dict(agreement=1.0, ari=1.0, nmi=1.0)
    assert compare.scores(np.array([[1]])) == dict(agreement=1.0, ari=1.0, nmi=1.0)


def test_ari_equals_a_hand_computed_value():
    # rows (3, 3), columns (3, 3), n = 6
    T = np.array([[2, 1], [1, 2]])
    # sum C(nij, 2) = 2; sum rows = 6; sum columns = 6; C(6, 2) = 15; expected = 36 / 15 = 2.4; max = 6
    assert compare.scores(T)["ari"] == pytest.approx((2 - 2.4) / (6 - 2.4), abs=1e-12)


def test_match_states_appends_the_unmatched_columns():
    T = np.array([[0, 9, 0, 1],
                  [0, 0, 2, 8]])            # KB = 4 > KA = 2: column 1 -> state 0, column 3 -> state 1; 0 and 2 -> 2, 3
    assert compare.match_states(T).tolist() == [2, 0, 3, 1]
    P = compare.permute_columns(T, [2, 0, 3, 1])
    assert P.tolist() == [[9, 1, 0, 0], [0, 8, 0, 2]]
    assert compare.match_states(T.T).tolist() == [1, 3]        # KB < KA: every column matched


# ---- refusals ahead of any library call -------------------------------------------------------------------------------------
def _mat(path, **fields):
    scipy.io.savemat(str(path), fields)
    return str(path)


LV = np.array([[6, 0, 6, 3, 3, 0, 0, 0, 1, 1]])


def test_compare_files_refuses_what_cannot_be_compared(tmp_path):
    sv = np.zeros((1, 6), dtype=np.int64)
    a = _mat(tmp_path / "a.mat", state_vec=sv, len_vec=LV)
    other = LV.copy()
    other[0, 9] = 2
    b = _mat(tmp_path / "b.mat", state_vec=sv, len_vec=other)
    with pytest.raises(ValueError, match="same regions"):
        compare.compare_files(a, b, str(tmp_path), 50000)
    c = _mat(tmp_path / "c.mat", state_vec=sv, len_vec=LV)
    with pytest.raises(ValueError, match="state_vec_smooth"):
        compare.compare_files(a, c, str(tmp_path), 50000, field="state_vec_smooth")
    with pytest.raises(ValueError, match="conf"):
        compare.compare_files(a, c, str(tmp_path), 50000, min_conf=0.5)
    d = _mat(tmp_path / "d.mat", state_vec=sv, len_vec=LV, conf=np.ones((1, 6), dtype=np.float32))
    with pytest.raises(ValueError, match="conf"):
        compare.compare_files(d, c, str(tmp_path), 50000, min_conf=0.5)     # conf in one file only
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("compare_")]


def test_compare_states_refuses_bad_arguments_before_the_library():
    z = np.zeros(6, dtype=np.int64)
    with pytest.raises(ValueError):
        compare.compare_states(z, z[:5], LV)
    with pytest.raises(ValueError):
        compare.compare_states(z, z, LV, conf_a=np.ones(6))
    with pytest.raises(ValueError):
        compare.compare_states(z, z, LV, min_conf=0.5)
    with pytest.raises(ValueError):
        compare.compare_states(z, z, LV, min_area=0)


def test_no_host_fallback():
    from phylo_hmrf_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")                     # (tests/test_gpu_compare.py runs the call there)
    z = np.array([0, 1, 1, 0])
    with pytest.raises(RuntimeError):
        compare.contingency(z, z)
    with pytest.raises(RuntimeError):
        compare.compare_states(np.zeros(6, dtype=np.int64), np.zeros(6, dtype=np.int64), LV)


def _cli(**extra):
    import phylo_hmrf as cli
    return cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", "unused", quiet="1", **extra)


@pytest.mark.parametrize("extra", [
    dict(compare="a.mat"),
    dict(compare_with="b.mat"),
    dict(compare="a.mat", compare_with="b.mat", segment="m.npz"),
    dict(compare="a.mat", compare_with="b.mat", postprocess="x.mat"),
    dict(compare="a.mat", compare_with="b.mat", ancestral="posterior"),
    dict(compare="a.mat", compare_with="b.mat", save_model="m.npz"),
    dict(compare="a.mat", compare_with="b.mat", filter_device="1"),
    dict(compare="a.mat", compare_with="b.mat", compare_field="top"),
    dict(compare="a.mat", compare_with="b.mat", compare_match="2"),
])
def test_cli_refusals(extra):
    with pytest.raises(SystemExit) as e:
        _cli(**extra)
    assert "--compare" in str(e.value)
    assert not os.path.exists("unused")


def test_cli_parses_the_options_with_their_defaults():
    import phylo_hmrf as cli
    o = cli.parse_args(["--compare", "a.mat", "--compare_with", "b.mat"])
    assert (o.compare, o.compare_with, o.compare_field, o.compare_match, o.compare_min_conf, o.compare_area) == \
        ("a.mat", "b.mat", "state_vec", "0", "0", "-1")
    o = cli.parse_args([])
    assert (o.compare, o.compare_with) == ("", "")


def test_header_keeps_its_version_and_documents_both_calls():
    from phylo_hmrf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert "#define PHMRF_VERSION 127\n" in txt and _lib.ABI_VERSION == 127
    assert "#define PHMRF_DIFF_BANDS 32\n" in txt and "#define PHMRF_DOMAIN_COLS 12\n" in txt
    assert compare.DIFF_BANDS == 32 and compare.DOMAIN_COLS == 12
    for name in ("phmrf_label_contingency", "phmrf_diff_domains"):
        assert "PHMRF_API int %s(" % name in txt and name in _lib.SIGNATURES
        assert txt.count(name) >= 2                         # declared and described
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "compare.hip")).read()
    assert "CONT_GRID_CAP = %d;" % compare.CONTINGENCY_GRID_CAP in src
    assert "CONT_PER_TRIP = %d;" % compare.CONTINGENCY_PER_TRIP in src
