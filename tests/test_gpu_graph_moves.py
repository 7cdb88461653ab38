"""GPU: the move kernels OFF the complete stencil grid, label for label against the float64 move model
(oracle/mrf_moves.py) on the exact-arithmetic cases of tests/graph_move_cases.py:

  graphs that are no grid   icm_kernel over the host's greedy colouring, the adjacency-row component kernels (rows of width
                            4, 8, 12, 16 and 64), comp_table_kernel at every row-load width, chain_kernel on the path families
                            (read back through phmrf_block_get_chain_segments and checked to be safe), the solve;
  incomplete grids          grid blocks whose edge list is a subset of the stencil: the same block calls as the grid tests of
                            tests/test_gpu_estep.py, against the models on the incomplete edge list.

Every case is an integer problem (f32 arithmetic exact, component decisions safe from the margin: graph_move_cases.py), so
"equal" below means equal, and energies are compared at 1e-9."""
import numpy as np
import pytest

from oracle import mrf_moves as M
from tests import graph_move_cases as C

pytestmark = pytest.mark.gpu

GENERAL = C.general_names()
GRIDS = C.grid_names()
WITH_PATHS = [k for k in GENERAL if k != "tiny-n1-K2"]


def _case(name):
    return C.grid_cases()[name] if name in GRIDS else C.general_cases()[name]


def _block(c, labels=None):
    from phylo_hmrf_amd import Block
    b = Block(c.n, 2, c.K)
    b.set_graph(c.eid, c.w)
    if c.grid is not None:
        b.set_grid(*c.grid)
    b.set_logprob(c.lp)
    if labels is not None:
        b.set_labels(labels)
    return b


def _energy(c, lab):
    return M.energy(c.g, c.un, np.asarray(lab, dtype=np.int64), c.beta)[0]


def _icm_sweeps(c):
    col, ncol = c.colours()
    b = _block(c, c.init)
    nbr, _ = b.get_adjacency()
    assert nbr.shape[1] == c.D                                   # the row width the case was built for
    lab = c.init.copy()
    for sweep in range(C.N_ICM_SWEEPS):
        ch_ref = M.icm_sweep(c.g, c.un, lab, c.beta, col, ncol)
        ch = b.icm_sweep(c.beta)
        got = b.get_labels()
        assert np.array_equal(got, lab), (sweep, int((got != lab).sum()))
        assert ch == ch_ref
    np.testing.assert_allclose(b.energy(c.beta)[0], _energy(c, lab), rtol=1e-9)
    b.close()


def _component_passes(c, start, prepare=None):
    """N_COMPONENT_PASSES passes from `start`; prepare: None, "kept" (prepare_components on the labels the pass then finds)
    or "replaced" (prepared on other labels, `start` installed afterwards)"""
    b = _block(c, c.init if prepare == "replaced" else start)
    if prepare:
        b.prepare_components()
    if prepare == "replaced":
        b.set_labels(start)
    lab = start.copy()
    total = 0
    for it in range(C.N_COMPONENT_PASSES):
        ch_ref = M.component_pass(c.g, c.un, lab, c.beta)
        ch = b.component_pass(c.beta)
        got = b.get_labels()
        assert np.array_equal(got, lab), (it, int((got != lab).sum()), ch, ch_ref)
        assert ch == ch_ref
        total += ch
    b.close()
    return total


# ------------------------------------------------------------------------------------------------ graphs that are no grid
@pytest.mark.parametrize("name", GENERAL)
def test_icm_sweeps_over_the_greedy_colouring_match_the_move_model(name):
    _icm_sweeps(_case(name))


@pytest.mark.parametrize("name", GENERAL)
def test_component_passes_on_adjacency_rows_match_the_move_model(name):
    c = _case(name)
    assert _component_passes(c, c.comp_start) > 0


@pytest.mark.parametrize("name", ["knn-k8-n2999-K6", "path-n2500-K3", "33x70-rand15"])
def test_deterministic_mode_gives_the_same_moves(name, monkeypatch):
    """PHMRF_DETERMINISTIC=1 (read when a block is created): the 2^-16 fixed-point component table decides as the model"""
    monkeypatch.setenv("PHMRF_DETERMINISTIC", "1")
    c = _case(name)
    assert _component_passes(c, c.comp_start) > 0
    _icm_sweeps(c)


@pytest.mark.parametrize("name", ["knn-k4-n3001-K3", "33x70-rand40"])
@pytest.mark.parametrize("prepare", ["kept", "replaced"])
def test_prepared_components_give_the_unprepared_passes(name, prepare):
    c = _case(name)
    assert not np.array_equal(c.init, c.comp_start)
    assert _component_passes(c, c.comp_start, prepare) > 0


def _launches(b):
    """every launch of the chain kernel of a block -> {(family, phase, colour): list of node arrays}"""
    out = {}
    for family, ncol in enumerate(b.chain_family_info()):
        for phase in (0, 1):
            for colour in range(ncol):
                start, length, nodes = b.chain_segments(family, phase, colour)
                assert len(start) == len(length)
                assert np.all(start >= 0) and np.all(start.astype(np.int64) + length <= len(nodes))
                out[(family, phase, colour)] = [nodes[s:s + ln].astype(np.int64) for s, ln in zip(start, length)]
    return out


@pytest.mark.parametrize("name", WITH_PATHS)
def test_path_families_are_induced_paths_that_never_touch(name):
    """What makes the path moves safe: every segment of a launch is an induced path of 2 .. 63 nodes, no node occurs twice in
    a launch and no edge joins two of its segments.  The tables are built from fixed seeds: two blocks on one graph agree."""
    c = _case(name)
    b, b2 = _block(c, c.init), _block(c, c.init)
    assert b.chain_family_info() == [3, 3, 3, 3]
    launches = _launches(b)
    assert len(launches) == 4 * 2 * 3
    covered = np.zeros(c.n, dtype=bool)
    for key, segs in launches.items():
        assert not C.launch_violations(c.g, segs, 2, 63), (key, C.launch_violations(c.g, segs, 2, 63)[:3])
        for s in segs:
            covered[s] = True
    # (what no path covers keeps ICM and the component moves: nodes without a neighbour, for one)
    assert covered[np.diff(c.g.row_ptr) > 0].mean() > 0.8
    other = _launches(b2)
    assert sorted(other) == sorted(launches)
    for key, segs in launches.items():
        assert len(segs) == len(other[key]) and all(np.array_equal(x, y) for x, y in zip(segs, other[key])), key
    b.close()
    b2.close()


def test_a_single_node_has_no_path_families():
    from phylo_hmrf_amd import PhmrfError
    c = _case("tiny-n1-K2")
    b = _block(c, c.init)
    assert b.chain_family_info() == []
    with pytest.raises(PhmrfError) as ei:
        b.chain_sweep(c.beta, 0)
    assert ei.value.status == 1
    b.close()


def test_chain_sweep_without_a_grid_keeps_its_errors():
    from phylo_hmrf_amd import PhmrfError
    c = _case("hub-n301-K7")
    b = _block(c, c.init)
    for family in (-1, 4):
        with pytest.raises(PhmrfError) as ei:
            b.chain_sweep(c.beta, family)                       # no such chain family
        assert ei.value.status == 1
    for args in ((4, 0, 0), (0, 2, 0), (0, 0, 3), (0, 0, -1)):
        with pytest.raises(PhmrfError) as ei:
            b.chain_segments(*args)
        assert ei.value.status == 1
    assert b.chain_sweep(c.beta, 0) >= 0
    b.close()


@pytest.mark.parametrize("name", ["14x19-rand15", "40x40d-no-vertical", "33x70-nn4-rand20"])
def test_chain_segments_of_a_grid_block_are_the_models(name):
    c = _case(name)
    b = _block(c, c.init)
    nn = c.grid[3]
    assert b.chain_family_info() == ([2, 2, 3, 3] if nn == 8 else [2, 2])
    for (family, phase, colour), segs in _launches(b).items():
        ref = C.grid_segments(c, family, phase, colour)
        assert sorted(tuple(s.tolist()) for s in segs) == sorted(tuple(s.tolist()) for s in ref), (family, phase, colour)
    b.close()


def _chain_sweeps(c, launches_of):
    """every family's sweep against the model's chain move on the same segments, launch by launch in the library's order
    (cut phase 0 then 1, each over the colours).  As in the grid chain test the energies must be equal -- exact arithmetic,
    kernel and model may part only between labellings of equal energy -- and the next family continues from the GPU's
    labelling.  The kernel counts a label every time it changes it: where its labelling is the model's, the count is the
    model's; where only the energy is, every changed node must have changed once (the count is the number of labels that
    differ) -- and never fewer than that."""
    b = _block(c, c.init)
    launches = launches_of(b)
    lab = c.init.copy()
    moved = 0
    for family in range(len(b.chain_family_info())):
        before = lab.copy()
        e0 = _energy(c, before)
        ch_ref = 0
        for phase in (0, 1):
            for colour in sorted(k[2] for k in launches if k[0] == family and k[1] == phase):
                ch_ref += C.chain_move_on_segments(c, lab, launches[(family, phase, colour)])
        ch = b.chain_sweep(c.beta, family)
        got = b.get_labels().astype(np.int64)
        e_gpu, e_ref = _energy(c, got), _energy(c, lab)
        assert abs(e_gpu - e_ref) < 1e-9, (family, e_gpu, e_ref)
        assert e_gpu <= e0 + 1e-9, (family, e_gpu, e0)
        differ = int((got != before).sum())
        assert ch >= differ
        assert ch == (ch_ref if np.array_equal(got, lab) else differ), (family, ch, ch_ref, differ)
        moved += differ
        lab = got.copy()
    b.close()
    return moved


@pytest.mark.parametrize("name", WITH_PATHS)
def test_chain_sweeps_on_path_families_match_the_move_model(name):
    c = _case(name)
    assert _chain_sweeps(c, _launches) > 0 or c.n < 20


@pytest.mark.parametrize("name", ["knn-k4-n3001-K3", "hub-n301-K7"])
def test_solve_without_a_grid_ends_at_a_fixed_point(name):
    c = _case(name)
    b = _block(c, c.init)
    res = b.solve(c.beta)
    lab = b.get_labels()
    assert res["converged"]
    assert _energy(c, lab) <= _energy(c, c.init) + 1e-9
    np.testing.assert_allclose(res["energy"], _energy(c, lab), rtol=1e-9)
    assert b.icm_sweep(c.beta) == 0 and b.component_pass(c.beta) == 0
    assert np.array_equal(b.get_labels(), lab)
    b.close()


# ------------------------------------------------------------------------------------------------ incomplete grids
@pytest.mark.parametrize("name", GRIDS)
def test_incomplete_grid_component_passes_match_the_move_model(name):
    c = _case(name)
    assert _component_passes(c, c.comp_start) > 0


@pytest.mark.parametrize("name", GRIDS)
def test_incomplete_grid_icm_sweeps_match_the_move_model(name):
    _icm_sweeps(_case(name))


@pytest.mark.parametrize("name", GRIDS)
def test_incomplete_grid_strip_passes_match_the_move_model(name):
    """fusion with the best alternatives and one label's expansion in both orientations, then every label's expansion in
    one launch"""
    c = _case(name)
    H, W, diagonal, _ = c.grid
    b = _block(c, c.init)
    lab = c.init.copy()
    for it, (orient, sr, sc, alpha) in enumerate([(0, 0, 0, -1), (1, 3, 17, -1), (0, 2, 40, 1), (1, 5, 63, 0)]):
        prop = M.best_alternative(c.g, c.un, lab, c.beta) if alpha < 0 else np.full(c.n, alpha)
        ch_ref = M.strip_fusion(c.g, c.un, lab, prop, c.beta, H, W, diagonal, orient, sr, sc)
        ch = b.strip_pass(c.beta, orient, sr, sc, alpha)
        got = b.get_labels()
        assert np.array_equal(got, lab), (it, int((got != lab).sum()))
        assert ch == ch_ref
    for orient, sr, sc in ((0, 4, 21), (1, 0, 42)):
        ch_ref = 0
        for alpha in range(c.K):
            ch_ref += M.strip_fusion(c.g, c.un, lab, np.full(c.n, alpha), c.beta, H, W, diagonal, orient, sr, sc)
        ch = b.strip_multi_pass(c.beta, orient, sr, sc)
        got = b.get_labels()
        assert np.array_equal(got, lab), (orient, int((got != lab).sum()))
        assert ch == ch_ref
    b.close()


def _grid_launches(c):
    nn = c.grid[3]
    return lambda b: {(f, p, col): C.grid_segments(c, f, p, col) for f in range(4 if nn == 8 else 2) for p in (0, 1)
                      for col in range(2 if f < 2 else 3)}


@pytest.mark.parametrize("name", GRIDS)
def test_incomplete_grid_chain_sweeps_match_the_move_model(name):
    c = _case(name)
    assert _chain_sweeps(c, _grid_launches(c)) > 0


@pytest.mark.parametrize("name", ["33x70-rand15", "40x40d-rand40"])
def test_incomplete_grid_coarse_pass_matches_the_move_model(name):
    c = _case(name)
    H, W, diagonal, _ = c.grid
    b = _block(c, c.init)
    lab = c.init.copy()
    total = 0
    for it, (off, alpha, sr, sc) in enumerate([(0, 1, 0, 0), (1, 2, 5, 63), (0, 0, 3, 21)]):
        e0 = _energy(c, lab)
        ch_ref = M.coarse_expansion(c.g, c.un, lab, c.beta, H, W, diagonal, 2, off, alpha, sr, sc)
        ch = b.coarse_pass(c.beta, 2, off, alpha, sr, sc)
        got = b.get_labels()
        assert _energy(c, lab) <= e0 + 1e-9
        assert np.array_equal(got, lab), (it, int((got != lab).sum()))
        assert ch == ch_ref
        total += ch
    assert total > 0
    b.close()


@pytest.mark.parametrize("name", GRIDS)
def test_incomplete_grid_moves_never_raise_the_energy_and_the_solve_converges(name):
    """the float64 energy of the labels after every move type, and after the solve to the exact fixed point, is never above
    the energy before it"""
    c = _case(name)
    nn = c.grid[3]
    b = _block(c, c.init)
    e = [_energy(c, c.init)]

    def after(what):
        e.append(_energy(c, b.get_labels()))
        assert e[-1] <= e[-2] + 1e-9, (what, e[-2], e[-1])

    for rnd in range(2):
        b.component_pass(c.beta)
        after("component")
        b.icm_sweep(c.beta)
        after("icm")
        for family in range(4 if nn == 8 else 2):
            b.chain_sweep(c.beta, family)
            after("chain %d" % family)
        for orient in (0, 1):
            for alpha in (-1, rnd):
                b.strip_pass(c.beta, orient, (2 * rnd + orient) % 6, (11 * rnd + 5) % 64, alpha)
                after("strip %d %d" % (orient, alpha))
            b.strip_multi_pass(c.beta, orient, (3 + rnd) % 6, 40)
            after("strip multi %d" % orient)
        b.coarse_pass(c.beta, 2, rnd, rnd + 1, 1, 7)
        after("coarse")
    np.testing.assert_allclose(b.energy(c.beta)[0], e[-1], rtol=1e-9)
    res = b.solve(c.beta, energy_tol_ppb=0)
    after("solve")
    assert res["converged"]
    np.testing.assert_allclose(res["energy"], e[-1], rtol=1e-9)
    b.close()


@pytest.mark.parametrize("name", ["14x19-rand15", "33x70-rand15"])
def test_cut_general_graph_takes_an_incomplete_grid_for_a_grid(name):
    """pygco_compat.infer_grid declares such a list a grid on its own: the drop-in call must still return a labelling at or
    below the energy of the labels it was given"""
    import warnings
    from phylo_hmrf_amd import pygco_compat
    c = _case(name)
    b = _block(C.Case(name, c.n, c.K, c.beta, c.eid, c.w, c.un, c.init), c.init)          # (no grid declared)
    assert pygco_compat.infer_grid(b, c.n, c.eid) == c.grid
    b.close()
    pairwise = c.beta * (1.0 - np.eye(c.K))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                                     # (no "not a grid" warning)
        lab = pygco_compat.cut_general_graph(c.eid, c.w, c.un, pairwise, n_iter=-1, algorithm="swap", init_labels=c.init)
    assert lab.shape == (c.n,) and lab.min() >= 0 and lab.max() < c.K
    assert _energy(c, lab) <= _energy(c, c.init) + 1e-9
