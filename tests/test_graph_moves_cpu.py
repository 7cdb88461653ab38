"""CPU: the cases of tests/graph_move_cases.py are what they claim and discriminate; the helpers the GPU tests of
tests/test_gpu_graph_moves.py lean on are right.  No GPU, no library call."""
import numpy as np
import pytest

from oracle import mrf_moves as M
from tests import graph_move_cases as C

GENERAL = C.general_names()
GRIDS = C.grid_names()


def _general(name):
    return C.general_cases()[name]


def _grid(name):
    return C.grid_cases()[name]


def _case(name):
    return _grid(name) if name in GRIDS else _general(name)


def test_case_lists_are_the_builders_lists():
    assert list(C.general_cases()) == GENERAL and list(C.grid_cases()) == GRIDS


def test_general_cases_reach_the_branches_they_are_for():
    cases = C.general_cases()
    assert sorted(set(c.K for c in cases.values())) == [2, 3, 4, 6, 7, 64]
    assert all(c.n % 64 and c.n <= 5000 for c in cases.values())
    assert {cases[k].D for k in GENERAL if k.startswith("knn")} <= {12, 16} and cases["knn-k8-n2999-K6"].D == 16
    assert cases["hub-n301-K7"].D == 64 == cases["hub-n301-K7"].max_degree            # the documented limit, not beyond it
    assert cases["deg4-n1003-K2"].D == 4 and cases["deg4-n1003-K2"].max_degree == 4
    sparse = cases["sparse-n5000-K4"]
    deg = np.diff(sparse.g.row_ptr)
    assert (deg == 0).sum() > 50 and abs(deg.mean() - 3.0) < 0.2 and sparse.D > 8
    assert [cases[k].n for k in GENERAL if k.startswith("tiny")] == [1, 2, 3] and len(cases["tiny-n1-K2"].eid) == 0
    # the component passes have components to move, on every kind of graph
    for name in GENERAL:
        lab = cases[name].comp_start.copy()
        assert M.component_pass(cases[name].g, cases[name].un, lab, cases[name].beta) > 0, name


@pytest.mark.parametrize("name", GENERAL)
def test_replica_of_the_greedy_colouring_is_a_proper_colouring(name):
    c = _general(name)
    col, ncol = C.greedy_colouring(c.g)
    assert col.min() == 0 and col.max() == ncol - 1 and ncol <= c.max_degree + 1
    assert np.all(col[c.eid[:, 0]] != col[c.eid[:, 1]])
    # greedy in index order: no node could have taken a smaller colour given its smaller neighbours
    for i in range(c.n):
        row = c.g.col[c.g.row_ptr[i]:c.g.row_ptr[i + 1]]
        assert set(range(col[i])) <= set(col[row[row < i]].tolist()), i


def test_path_case_puts_run_boundaries_where_it_claims():
    lab, starts = C.path_run_labels(3)
    c = _general("path-n2500-K3")
    assert np.array_equal(c.init, lab) and np.array_equal(c.comp_start, lab)
    # the starts of all maximal runs of equal label, as cc_init_kernel sees them (i - 1 is on every node's row)
    assert np.all(c.eid[np.flatnonzero(c.eid[:, 1] - c.eid[:, 0] == 1)][:, 0] == np.arange(c.n - 1))
    run_starts = np.concatenate([[0], np.flatnonzero(np.diff(lab)) + 1])
    assert np.array_equal(run_starts, starts)
    lengths = np.diff(np.concatenate([run_starts, [c.n]]))
    for start, ln in C.PATH_RUNS:
        assert lengths[np.searchsorted(run_starts, start)] == ln and run_starts[np.searchsorted(run_starts, start)] == start
    assert sorted(ln for _, ln in C.PATH_RUNS) == sorted(C.PATH_RUN_LENGTHS)
    for (mod, res), claimed in C.PATH_CLAIMS.items():
        assert claimed and all(s % mod == res and s in run_starts for s in claimed), (mod, res)
    assert sorted(set(m for m, _ in C.PATH_CLAIMS)) == [64, 256] and sorted(set(r for _, r in C.PATH_CLAIMS)) == [0, 1, 63, 255]
    # runs that cross a wave chunk and a workgroup of the init kernel, and one that spans several workgroups
    assert any(s // 64 != (s + ln - 1) // 64 for s, ln in C.PATH_RUNS) and any(s // 256 + 2 <= (s + ln - 1) // 256 for s, ln in C.PATH_RUNS)


def _energy(c, lab):
    return M.energy(c.g, c.un, lab, c.beta)[0]


@pytest.mark.parametrize("name", GENERAL + GRIDS)
def test_model_moves_never_raise_the_energy(name):
    """ICM, component pass, chain move (and on grids strip fusion) of the float64 model on every case, incomplete grids
    included: the models take a missing edge as weight 0."""
    c = _case(name)
    col, ncol = c.colours()
    lab = c.init.copy()
    e = _energy(c, lab)

    def step(what, changed):
        nonlocal e
        e2 = _energy(c, lab)
        assert e2 <= e + 1e-9, (what, e, e2)
        assert changed > 0 or e2 == e, what
        e = e2

    for _ in range(2):
        before = lab.copy()
        ch = M.icm_sweep(c.g, c.un, lab, c.beta, col, ncol)
        assert ch == (lab != before).sum()
        step("icm", ch)
        before = lab.copy()
        ch = M.component_pass(c.g, c.un, lab, c.beta)
        assert ch == (lab != before).sum()
        step("component", ch)
        if c.grid is None:
            segs = C.greedy_induced_paths(c.g, np.random.default_rng(7))
            assert not C.launch_violations(c.g, segs)
            step("chain", C.chain_move_on_segments(c, lab, segs))
        else:
            H, W, diagonal, nn = c.grid
            for family in range(4 if nn == 8 else 2):
                for phase in (0, 1):
                    for colour in range(2 if family < 2 else 3):
                        step("chain", C.chain_move_on_segments(c, lab, C.grid_segments(c, family, phase, colour)))
            for orient, sr, sc, alpha in ((0, 0, 0, -1), (1, 3, 17, 1)):
                prop = M.best_alternative(c.g, c.un, lab, c.beta) if alpha < 0 else np.full(c.n, alpha)
                step("strip", M.strip_fusion(c.g, c.un, lab, prop, c.beta, H, W, diagonal, orient, sr, sc))


@pytest.mark.parametrize("name", GRIDS)
def test_incomplete_grids_are_incomplete_and_discriminate(name):
    """Every incomplete case has a component of equal label that hangs together only by an edge a complete-stencil argument
    would skip: the components over the on-file edges differ from those of the union kernel's shortcut (stated in its own
    comment) -- so a component kernel that keeps the shortcut on such a list gives other components, and the GPU cases see
    it.  Which form of the shortcut can differ depends on what is gone:
      "largest"   (a linked-left node unions with its largest remaining smaller neighbour only) can part from the truth only
                  where a row can hold two smaller neighbours besides i - 1 of which the skipped one matters: the random
                  removals and the missing verticals of an 8-neighbour list.  With a whole direction gone, or with at most one
                  such neighbour per row (the 4-neighbour lists, horizontal + anti-diagonal), it is exact -- which is also
                  why the 4-neighbour form of the shortcut is sound on an incomplete 4-neighbour grid;
      "stencil8"  (the 8-neighbour refinement: a linked-left cell acts only on a third upper neighbour) parts from the truth
                  on every list declared with 8 neighbours."""
    c = _grid(name)
    H, W, diagonal, nn = c.grid
    n, full, _ = C.stencil_edges(H, W, diagonal, nn)
    assert n == c.n and len(c.eid) < len(full) == c.expected_edges
    assert set(map(tuple, c.eid.tolist())) < set(map(tuple, full.tolist()))
    removal = name.split("-", 1)[1]
    if removal in ("four-on-file", "horizontal-anti", "nn4-rand20"):
        assert c.D == 4
    truth = C.true_components(c, c.comp_start)
    largest = C.shortcut_components(c, c.comp_start, "largest")
    # a shortcut only ever unions along on-file edges of equal label: its components refine the true ones
    assert np.all(truth[largest] == truth) and np.all(largest >= truth)
    if nn == 4:
        assert np.array_equal(largest, truth)
        return
    stencil8 = C.shortcut_components(c, c.comp_start, "stencil8")
    assert np.all(truth[stencil8] == truth)
    assert not np.array_equal(stencil8, truth), name
    if removal.startswith("rand") or removal == "no-vertical":
        assert not np.array_equal(largest, truth), name
    # on the complete stencil both forms of the shortcut are exact (the discrimination is the missing edges' doing)
    w = np.ones(len(full))
    whole = C.Case(name + "-complete", c.n, c.K, c.beta, full, w, c.un, c.init, grid=c.grid)
    whole_truth = C.true_components(whole, c.comp_start)
    assert np.array_equal(C.shortcut_components(whole, c.comp_start, "largest"), whole_truth)
    assert np.array_equal(C.shortcut_components(whole, c.comp_start, "stencil8"), whole_truth)


def test_launch_violations_finds_every_kind_of_unsafe_segment():
    c = _general("knn-k4-n3001-K3")
    g = c.g
    segs = C.greedy_induced_paths(g, np.random.default_rng(3))
    assert len(segs) > 50 and max(len(s) for s in segs) > 5 and not C.launch_violations(g, segs)
    long = max(segs, key=len)

    def kinds(segments, **kw):
        return sorted(set(v[0] for v in C.launch_violations(g, segments, **kw)))

    assert kinds([long[:1]]) == ["length"]
    assert kinds([long], max_len=len(long) - 1) == ["length"]
    assert "node twice" in kinds([long, long[:2]])
    i = int(np.flatnonzero(np.diff(g.row_ptr) >= 3)[0])                 # a node and two of its neighbours, out of order
    nb = g.col[g.row_ptr[i]:g.row_ptr[i + 1]]
    assert "consecutive nodes not adjacent" in kinds([np.array([nb[0], nb[1], i])]) or \
        "edge between nodes of a segment that are not consecutive" in kinds([np.array([nb[0], nb[1], i])])
    # a triangle-free detour: a path that closes a cycle is not induced
    tri = None
    for a, b in c.eid:
        common = np.intersect1d(g.col[g.row_ptr[a]:g.row_ptr[a + 1]], g.col[g.row_ptr[b]:g.row_ptr[b + 1]])
        if len(common):
            tri = np.array([a, b, common[0]])
            break
    assert tri is not None and kinds([tri]) == ["edge between nodes of a segment that are not consecutive"]
    a, b = c.eid[0]
    na = [u for u in g.col[g.row_ptr[a]:g.row_ptr[a + 1]] if u != b and u not in g.col[g.row_ptr[b]:g.row_ptr[b + 1]]][0]
    nbb = [u for u in g.col[g.row_ptr[b]:g.row_ptr[b + 1]] if u != a and u != na and u not in g.col[g.row_ptr[a]:g.row_ptr[a + 1]]
           and u not in g.col[g.row_ptr[na]:g.row_ptr[na + 1]]][0]
    assert kinds([np.array([na, a]), np.array([b, nbb])]) == ["edge between two segments"]


def test_grid_segments_are_the_cuts_of_the_models_chains():
    c = _grid("33x70-rand15")
    H, W, diagonal, nn = c.grid
    whole = M.Graph(c.n, C.stencil_edges(H, W, diagonal, 8)[1], np.ones(c.expected_edges))
    for family in range(4):
        for phase in (0, 1):
            seen = np.zeros(c.n, dtype=int)
            for colour in range(2 if family < 2 else 3):
                segs = C.grid_segments(c, family, phase, colour)
                assert not C.launch_violations(whole, segs, min_len=1)          # safe on the complete stencil, hence on a subset
                for s in segs:
                    seen[s] += 1
            # every node but the separators, once
            assert seen.max() == 1 and (seen == 0).sum() == sum(max(0, (len(ch) - (32 if phase else 64)) // 64 + 1)
                                                                for ch in M.chain_families(H, W, diagonal, 8)[family][0]
                                                                if len(ch) > (31 if phase else 63))
