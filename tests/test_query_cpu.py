"""CPU: the host side of the interval-pair query (phylo_hmrf_amd.query): the reduction of a query's bin pairs to signed
rectangles, hand-worked and against the set definition of tests/query_reference.py, the bin rule and the readers, the controls,
the text columns, the command line's checks and the declaration of phmrf_rect_states.  No GPU call is made here."""
import os
import re

import numpy as np
import pytest

from phylo_hmrf_amd import query
from tests import query_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_gpu_pileup.py's layout: chromosome 1 = two diagonal regions (bins 2 .. 31 and 32 .. 56) and the off-diagonal region
# between them (rows 2 .. 31, columns 32 .. 56); chromosome 2 = one diagonal region (bins 0 .. 11)
SHAPES = [(30, 30, 1, 2, 2, 1), (30, 25, 0, 2, 32, 1), (25, 25, 1, 32, 32, 1), (12, 12, 1, 0, 0, 2)]
SEAM = 32
K_MAP = 6


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


def _one_diagonal(side):
    """a diagonal region at bin 0 whose node v is in state v: a histogram names the nodes"""
    L, n = _len_vec([(side, side, 1, 0, 0, 1)])
    return np.arange(n), L, n


def _nodes(side, cells):
    I, J = np.triu_indices(side)
    where = {(int(i), int(j)): v for v, (i, j) in enumerate(zip(I, J))}
    return sorted(where[c] for c in cells)


def _host_counts(s, L, q, K):
    """the module's rectangles counted by the reference's rectangle loop, region by region"""
    q = np.asarray(q, dtype=np.int64).reshape(-1, 5)
    total = np.zeros((q.shape[0], K), dtype=np.int64)
    per_region = query.rectangles(q, L)
    for row, (rect, slot, minus) in zip(L, per_region):
        assert rect.dtype == np.int32 and slot.dtype == np.int32 and minus.dtype == np.uint8 and rect.shape == (slot.shape[0], 4)
        total += R.table(s[row[1]:row[2]], None, int(row[3]), int(row[4]), int(row[8]), K, rect, slot, minus, q.shape[0])[0]
    return total, per_region


# ---- hand-worked ------------------------------------------------------------------------------------------------------------
def test_a_bed_interval_on_a_small_diagonal_region():
    s, L, n = _one_diagonal(4)
    counts, per_region = _host_counts(s, L, [[1, 1, 3, 1, 3]], n)
    assert per_region[0][0].tolist() == [[1, 3, 1, 3]] and per_region[0][1].tolist() == [0] and per_region[0][2].tolist() == [0]
    assert np.flatnonzero(counts[0]).tolist() == _nodes(4, [(1, 1), (1, 2), (2, 2)]) == [4, 5, 7] and counts.sum() == 3
    assert query.n_pairs([[1, 1, 3, 1, 3]]).tolist() == [3]


def test_an_interval_inside_the_other():
    """A = [0, 10), B = [2, 4): A x B clipped to the upper triangle alone loses {3, 8}, which is stored as (3, 8) in B x A"""
    s, L, n = _one_diagonal(10)
    counts, per_region = _host_counts(s, L, [[1, 0, 10, 2, 4]], n)
    assert per_region[0][0].tolist() == [[0, 10, 2, 4], [2, 4, 0, 10], [2, 4, 2, 4]] and per_region[0][2].tolist() == [0, 0, 1]
    assert counts[0, _nodes(10, [(3, 8)])[0]] == 1
    # 2 pairs with each of 0 .. 9, {2, 3} once: 19
    want = _nodes(10, [(0, 2), (0, 3), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)] + [(2, j) for j in range(4, 10)] + [(3, j) for j in range(4, 10)])
    assert np.flatnonzero(counts[0]).tolist() == want and counts.max() == 1 and counts.sum() == 19 == query.n_pairs([[1, 0, 10, 2, 4]])[0]
    swapped, _ = _host_counts(s, L, [[1, 2, 4, 0, 10]], n)
    assert np.array_equal(swapped, counts)


def test_intervals_that_overlap_partly():
    """A = [2, 6), B = [4, 9): 4 x 5 - 1 = 19 pairs; A x B holds 19 stored nodes, B x A the 3 of (4, 4), (4, 5), (5, 5), which
    (A and B)^2 takes off again"""
    s, L, n = _one_diagonal(12)
    counts, per_region = _host_counts(s, L, [[1, 2, 6, 4, 9]], n)
    assert per_region[0][0].tolist() == [[2, 6, 4, 9], [4, 9, 2, 6], [4, 6, 4, 6]] and per_region[0][2].tolist() == [0, 0, 1]
    want = [(i, j) for i in range(2, 6) for j in range(4, 9) if i <= j]
    assert len(want) == 19 and np.flatnonzero(counts[0]).tolist() == _nodes(12, want) and counts.max() == 1 and counts.min() == 0
    assert query.n_pairs([[1, 2, 6, 4, 9]]).tolist() == [19]


def test_an_interval_across_the_seam():
    """A = B = bins 28 .. 35: 36 pairs, 10 in the first diagonal region, 16 in the off-diagonal one, 10 in the second"""
    s, L = _genome()
    q = [[1, SEAM - 4, SEAM + 4, SEAM - 4, SEAM + 4]]
    counts, per_region = _host_counts(s, L, q, K_MAP)
    assert [p[0].tolist() for p in per_region] == [[[26, 30, 26, 30]], [[26, 30, 0, 4]], [[0, 4, 0, 4]], []]
    assert counts.sum() == 36 == query.n_pairs(q)[0]
    assert np.array_equal(counts, R.state_query(s, L, q, K_MAP)[0])


def test_an_off_diagonal_region_reached_through_its_mirror():
    """A = bins 40 .. 44 lies right of B = bins 5 .. 7: the region stores the pairs as (row in B, column in A)"""
    s, L = _genome()
    q = [[1, 40, 45, 5, 8]]
    counts, per_region = _host_counts(s, L, q, K_MAP)
    assert [p[0].tolist() for p in per_region] == [[], [[3, 6, 8, 13]], [], []] and per_region[1][2].tolist() == [0]
    assert counts.sum() == 15 == query.n_pairs(q)[0] and np.array_equal(counts, R.state_query(s, L, q, K_MAP)[0])


# ---- seeded -----------------------------------------------------------------------------------------------------------------
def _seeded_queries(rng, count, lo=-6, hi=66):
    a0, b0 = rng.integers(lo, hi, count), rng.integers(lo, hi, count)
    q = np.stack([rng.integers(1, 4, count), a0, a0 + rng.integers(0, 14, count), b0, b0 + rng.integers(0, 14, count)], axis=1)
    q[::7, 3:] = q[::7, 1:3]                                  # A == B
    q[3::11, 3] = q[3::11, 1] + 1                             # B inside or across the end of A
    q[3::11, 4] = np.maximum(q[3::11, 3], q[3::11, 2] - rng.integers(-2, 3, q[3::11].shape[0]))
    return q.astype(np.int64)


def test_n_pairs_against_the_listed_set():
    q = _seeded_queries(np.random.default_rng(1), 400)
    got = query.n_pairs(q)
    assert got.dtype == np.int64 and got.tolist() == [R.pairs_of(*row[1:]) for row in q.tolist()]
    assert query.n_pairs([[1, 0, 7, 0, 7], [1, 3, 3, 0, 9]]).tolist() == [28, 0]


def test_the_rectangles_are_the_set_definition():
    """inclusion-exclusion on the host: >= 1,000 seeded queries over the seam layout, negative and overhanging intervals, a
    chromosome the map does not hold"""
    s, L = _genome()
    q = _seeded_queries(np.random.default_rng(2), 1200)
    counts, per_region = _host_counts(s, L, q, K_MAP)
    want = R.state_query(s, L, q, K_MAP)[0]
    assert np.array_equal(counts, want), np.argwhere(counts != want)[:5].tolist()
    assert counts.min() >= 0 and np.all(counts.sum(axis=1) <= query.n_pairs(q)) and counts[q[:, 0] == 3].sum() == 0
    assert all(len(p[1]) <= 3 * 1200 for p in per_region) and counts.any()
    for row, (rect, slot, minus) in zip(L, per_region):       # nothing empty is submitted, nothing wholly below a diagonal
        assert np.all(rect[:, 1] > rect[:, 0]) and np.all(rect[:, 3] > rect[:, 2]) and rect.min(initial=0) >= 0
        assert np.all(rect[:, 1] <= row[3]) and np.all(rect[:, 3] <= row[4]) and (not row[8] or np.all(rect[:, 0] < rect[:, 3]))


def test_covered_queries_hold_every_pair():
    s, L = _genome()
    rng = np.random.default_rng(3)
    a0, b0 = rng.integers(2, 50, 300), rng.integers(2, 50, 300)
    q = np.stack([np.ones(300, dtype=np.int64), a0, a0 + rng.integers(1, 8, 300), b0, b0 + rng.integers(1, 8, 300)], axis=1)
    counts, _ = _host_counts(s, L, q, K_MAP)                  # chromosome 1's regions cover the bins 2 .. 56
    assert counts.sum(axis=1).tolist() == query.n_pairs(q).tolist()
    L2, n2 = _len_vec([(12, 12, 1, 0, 0, 2)])
    counts, _ = _host_counts(np.zeros(n2, dtype=np.int64), L2, [[2, 8, 16, 8, 16], [2, 0, 3, 20, 25]], 1)
    assert counts[:, 0].tolist() == [10, 0]                   # bins 12 .. 15 are in no region


# ---- the readers ------------------------------------------------------------------------------------------------------------
def _write(tmp_path, name, text):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def test_the_bin_rule(tmp_path):
    _, L = _genome()
    bed = _write(tmp_path, "a.bed", "chr1 50000 55000 anchor\nchr1 100000 200000\nchr1 70000 70000 point\nchr1 99999 100001\n")
    got = query.read_intervals(bed, L, 50000)
    # a 5 kb anchor keeps its bin; a stop on a bin edge ends there; start == stop is the bin of the point; 2 bp across an edge: 2 bins
    assert got["queries"].tolist() == [[1, 1, 2, 1, 2], [1, 2, 4, 2, 4], [1, 1, 2, 1, 2], [1, 1, 3, 1, 3]]
    assert got["names"] == ["anchor", ".", "point", "."] and got["skipped_lines"] == 0
    assert got["lines"][0] == ("chr1", 50000, 55000, 50000, 55000) and got["queries"].dtype == np.int64


def test_the_readers_names_skips_and_refusals(tmp_path):
    _, L = _genome()
    bed = _write(tmp_path, "t.bed", "# tads\n\nchr1\t100000\t250000\ttad1\nchrX 0 5 x\n2 0 100000\nchr9 5 10\n")
    got = query.read_intervals(bed, L, 50000)
    assert got["queries"].tolist() == [[1, 2, 5, 2, 5], [2, 0, 2, 0, 2]] and got["names"] == ["tad1", "."] and got["skipped_lines"] == 2
    bedpe = _write(tmp_path, "l.bedpe", "chr1 1400000 1405000 chr1 1700000 1750000 loop\nchr1 2000000 2050000 chr1 500000 550000\n"
                                        "chr1 0 5 chr2 0 5 across\nchr5 0 5 chr5 10 20\n")
    got = query.read_pairs(bedpe, L, 50000)
    assert got["queries"].tolist() == [[1, 28, 29, 34, 35], [1, 40, 41, 10, 11]] and got["names"] == ["loop", "."]
    assert got["skipped_lines"] == 2 and got["lines"][1] == ("chr1", 2000000, 2050000, 500000, 550000)
    empty = query.read_pairs(_write(tmp_path, "e.bedpe", "# nothing\n"), L, 50000)
    assert empty["queries"].shape == (0, 5) and empty["names"] == [] and empty["lines"] == []
    for name, text in (("m1.bed", "chr1 100\n"), ("m2.bed", "chr1 a 100\n"), ("m3.bed", "chr1 -5 100\n"), ("m4.bed", "chr1 200 100\n")):
        with pytest.raises(ValueError):
            query.read_intervals(_write(tmp_path, name, text), L, 50000)
    for name, text in (("m1.bedpe", "chr1 0 5 chr1 10\n"), ("m2.bedpe", "chr1 0 5 chr1 x 20\n"), ("m3.bedpe", "chr1 0 5 chr1 30 20\n"),
                       ("m4.bedpe", "chr1 0 5 chr1 -30 20\n")):
        with pytest.raises(ValueError):
            query.read_pairs(_write(tmp_path, name, text), L, 50000)
    with pytest.raises(ValueError):
        query.read_intervals(bed, L, 0)


def test_with_controls():
    q = np.array([[1, 10, 12, 30, 33], [1, 2, 5, 2, 5], [2, 40, 41, 3, 4]], dtype=np.int64)
    ctl, owner = query.with_controls(q, 3)
    assert ctl.tolist() == [[1, 7, 9, 27, 30], [1, 13, 15, 33, 36], [1, 5, 8, 5, 8], [2, 37, 38, 0, 1], [2, 43, 44, 6, 7]]
    assert owner.tolist() == [0, 0, 1, 2, 2] and owner.dtype == np.int64
    assert query.n_pairs(ctl).tolist() == [6, 6, 6, 1, 1]      # a shift along the diagonal keeps the shape
    assert query.control_counts(np.array([[1, 0], [2, 1], [0, 5], [1, 1], [1, 1]]), owner, 3).tolist() == [[3, 1], [0, 5], [2, 2]]
    with pytest.raises(ValueError):
        query.with_controls(q, 0)
    for bad in (np.zeros((2, 4), dtype=np.int64), np.zeros((2, 5)), [[1, 5, 4, 0, 1]], [[1, 0, 1, 0, 1 << 30]]):
        with pytest.raises(ValueError):
            query.n_pairs(bad)


def test_the_text_columns():
    lines = [("chr1", 100, 200, 300, 400), ("2", 0, 50, 0, 50), ("chr1", 5, 6, 5, 6)]
    counts = np.array([[1, 3, 0], [2, 0, 2], [0, 0, 0]])
    ctl = np.array([[2, 2, 0], [0, 0, 4], [1, 0, 0]])
    conf_sum = np.array([3 << 24, 1 << 24, 0], dtype=np.int64)
    out = query.query_lines(lines, ["loop", ".", "gap"], counts, [4, 6, 1], conf_sum, ctl)
    assert out[0] == ("#chrom\tstart1\tstop1\tstart2\tstop2\tname\tpairs\tcovered\tdominant_state\tshare\tentropy_bits\tmean_conf\t"
                      "control_total\tlog2_ratio\tstate_1\tstate_2\tstate_3\n")
    assert out[1] == "chr1\t100\t200\t300\t400\tloop\t4\t4\t2\t0.750000\t0.811278\t0.750000\t4\t0.5850\t1\t3\t0\n"
    assert out[2] == "2\t0\t50\t0\t50\t.\t6\t4\t1\t0.500000\t1.000000\t0.250000\t4\tnan\t2\t0\t2\n"       # the lowest state on a tie
    assert out[3] == "chr1\t5\t6\t5\t6\tgap\t1\t0\t0\t0.000000\t0.000000\tnan\t1\tnan\t0\t0\t0\n"
    plain = query.query_lines(lines, ["loop", ".", "gap"], counts, [4, 6, 1])
    assert plain[1] == "chr1\t100\t200\t300\t400\tloop\t4\t4\t2\t0.750000\t0.811278\tnan\t1\t3\t0\n" and len(plain) == 4
    assert query.mean_conf([1 << 23, 5], [1, 0]).tolist()[0] == 0.5 and np.isnan(query.mean_conf([1 << 23, 5], [1, 0])[1])


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_check_query():
    import phylo_hmrf as cli
    rest = ("", "", "", "", "", "", "", "", "", "", "", "0", "0")   # segment .. filter_device
    assert cli.check_query("", "", "", "state_vec", "0", "50000", *rest) is None
    assert cli.check_query("m.mat", "a.bed", "", "state_vec", "0", "50000", *rest) == 0
    assert cli.check_query("m.mat", "", "a.bedpe", "state_vec_smooth", "150000", "50000", *rest) == 3
    for args in (("", "a.bed", "", "state_vec", "0"), ("m.mat", "", "", "state_vec", "0"), ("m.mat", "a.bed", "b.bedpe", "state_vec", "0"),
                 ("m.mat", "a.bed", "", "conf", "0"), ("m.mat", "a.bed", "", "state_vec", "70000"), ("m.mat", "a.bed", "", "state_vec", "-50000")):
        with pytest.raises(SystemExit):
            cli.check_query(*args, "50000", *rest)
    names = ("segment", "postprocess", "compare", "domains", "render", "tracks", "enrich", "pileup", "consensus", "ancestral",
             "save_model", "profile", "filter_device")
    for at, name in enumerate(names):
        other = list(rest)
        other[at] = "1" if name in ("profile", "filter_device") else "x.mat"
        with pytest.raises(SystemExit) as e:
            cli.check_query("m.mat", "a.bed", "", "state_vec", "0", "50000", *other)
        assert "--query cannot be combined with --%s" % name in str(e.value)
    opts = cli.parse_args(["--query", "m.mat", "--query_bedpe", "l.bedpe", "--query_shift", "100000"])
    assert (opts.query, opts.query_bed, opts.query_bedpe, opts.query_field, opts.query_shift) == ("m.mat", "", "l.bedpe", "state_vec", "100000")


def test_every_other_mode_refuses_query():
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
    }
    for name, (check, args) in calls.items():
        check(*args)                                          # fine without --query, refused with it
        with pytest.raises(SystemExit) as e:
            check(*args, query="m.mat")
        assert "--query" in str(e.value), name


def test_the_entry_point_is_declared():
    from phylo_hmrf_amd import _lib
    header = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    m = re.search(r"PHMRF_API int phmrf_rect_states\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S)
    assert m and len(m.group(1).split(",")) == 14 == len(_lib.SIGNATURES["phmrf_rect_states"])
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "query.hip")).read()
    for name, value in (("RECT_TILE_H", query.TILE_H), ("RECT_TILE_W", query.TILE_W), ("RECT_VEC_MIN", query.VEC_MIN),
                        ("RECT_WAVES", query.WAVES), ("RECT_GRID_CAP", query.GRID_CAP)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name
    shared = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "interval_lists.h")).read()  # what pileup, query and aggregate compile
    assert "constexpr int COORD_LIMIT = 1 << 30;" in shared and query.COORD_LIMIT == 1 << 30 and '#include "interval_lists.h"' in src
    assert "query.hip" in open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "Makefile")).read()
