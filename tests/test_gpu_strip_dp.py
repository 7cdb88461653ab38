"""The profile DP behind the strip filter (strip.hip: dp_flagged) on inputs that force what the shapes of
tests/test_gpu_estep.py leave to chance: decisions recorded in every pass and chunk, isolated cells with dead chunks
between them, a window across a pass boundary, exact ties, a strip that moves for several labels in one launch -- each
case asserts from the NumPy move model that its input does what it claims, then compares the kernel label for label.
The last two tests hold the label hashes of seeded real-valued problems recorded before the DP was reworked
(tests/strip_dp_cases.py, tests/golden/strip_dp_labels.json)."""
import json
import os

import numpy as np
import pytest

from oracle import mrf_moves as M
from tests import strip_dp_cases as C
from tests.test_gpu_estep import _block, _integer_problem

pytestmark = pytest.mark.gpu

SH, SL = 5, 63
# one strip of 5 x 63 cells with its rim on all four sides: bands start at 6 b - shift_r and segments at 64 s - shift_c, so
# the cut (5, 63) puts the strip's first cell at (1, 1) of a 7 x 65 grid (orientation 1: of the 65 x 7 transpose)
ONE_STRIP_CUT = (5, 63)


def _one_strip(orient):
    H, W = (7, 65) if orient == 0 else (65, 7)
    return H, W


def _cell_node(orient, W, t):
    """node of cell t (column-major: t = 5 column + row) of the one strip"""
    cc, rr = divmod(t, SH)
    i, j = (1 + rr, 1 + cc) if orient == 0 else (1 + cc, 1 + rr)
    return i * W + j


def _forced_problem(seed, H, W, K, diagonal, movers, targets=None):
    """The integer problem of the move-model tests with decided outcomes: node i of `movers` gets its target label (default:
    its label + 1) at -30, its own label at 0 and every other label at 20; every other node its own label at -30 (its other
    unaries lie in [-2, 5.5]).  A node's pair terms change by at most 8 beta w = 8, so exactly the movers move, each once
    and straight to its target, whatever the order of the labels."""
    n, eid, w, lp, init = _integer_problem(seed, H, W, K, diagonal)
    un = -lp
    movers = np.asarray(movers, dtype=np.int64)
    tgt = (init + 1) % K
    if targets is not None:
        tgt[movers] = targets
    assert np.all(tgt[movers] != init[movers])
    stay = np.ones(n, dtype=bool)
    stay[movers] = False
    un[np.arange(n)[stay], init[stay]] = -30.0
    un[movers, :] = 20.0
    un[movers, init[movers]] = 0.0
    un[movers, tgt[movers]] = -30.0
    return n, eid, w, -un, init, tgt


def _run(entry, b, g, lp, lab, beta, H, W, diagonal, orient, cut, K, labels=None):
    """one fusion pass (entry 'fusion': strip_pass with alpha = -1) or every label's expansion in one launch ('multi') on the
    block and on the model (`labels`: of these labels only); -> (changed on the GPU, changed by the model per label or in all)"""
    sr, sc = cut
    if entry == "fusion":
        prop = M.best_alternative(g, -lp, lab, beta)
        ref = [M.strip_fusion(g, -lp, lab, prop, beta, H, W, diagonal, orient, sr, sc)]
        ch = b.strip_pass(beta, orient, sr, sc, -1)
    else:
        ref = [M.strip_fusion(g, -lp, lab, np.full(len(lab), a), beta, H, W, diagonal, orient, sr, sc)
               for a in (range(K) if labels is None else sorted(labels))]
        ch = b.strip_multi_pass(beta, orient, sr, sc, labels)
    return ch, ref


def _setup(n, K, eid, w, H, W, diagonal, lp, init):
    b = _block(n, 2, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 8)
    b.set_logprob(lp)
    b.set_labels(init)
    return b


WINDOWS = {"every cell": list(range(SH * SL)), "first and last": [0, SH * SL - 1], "across a pass": list(range(50, 81))}


@pytest.mark.parametrize("entry", ["fusion", "multi"])
@pytest.mark.parametrize("orient", [0, 1])
@pytest.mark.parametrize("window", list(WINDOWS))
def test_forced_windows_on_one_strip(window, orient, entry):
    """(a) every cell of the strip takes its proposal: decisions recorded in all five passes and all chunks, backtracked
    across every pass boundary; (b) exactly the first and the last cell move, dead chunks between them; (c) the window
    starts inside one pass and ends inside the next (cells 50 .. 80)."""
    K, beta = 4, 1.0
    H, W = _one_strip(orient)
    cells = WINDOWS[window]
    movers = [_cell_node(orient, W, t) for t in cells]
    n, eid, w, lp, init, tgt = _forced_problem(7 + orient, H, W, K, False, movers)
    g = M.Graph(n, eid, w)
    b = _setup(n, K, eid, w, H, W, False, lp, init)
    lab = init.astype(np.int64).copy()
    ch, ref = _run(entry, b, g, lp, lab, beta, H, W, False, orient, ONE_STRIP_CUT, K)
    # the case's precondition, from the model: one strip (the rim never moves), exactly these cells move, each to its proposal
    nodes, ncols = M.strip_node_table(H, W, False, orient, *ONE_STRIP_CUT)
    real = np.nonzero((nodes >= 0).any(axis=1))[0]
    assert len(real) == 1 and ncols[real[0]] == SL and int((nodes >= 0).sum()) == SH * SL
    assert sum(ref) == len(cells) and (window != "every cell" or sum(ref) == 315)
    assert sorted(np.nonzero(lab != init)[0]) == sorted(movers) and np.array_equal(lab[movers], tgt[movers])
    got = b.get_labels().astype(np.int64)
    assert np.array_equal(got, lab), int((got != lab).sum())
    assert ch == sum(ref)
    b.close()


@pytest.mark.parametrize("entry", ["fusion", "multi"])
@pytest.mark.parametrize("orient", [0, 1])
def test_all_ties_move_nothing(orient, entry):
    """(d) zero unary differences and zero weights: every proposal costs exactly what the label costs, the filter cannot
    settle the strip (cost 0 against cap 0), and the DP's tie rule keeps every cell."""
    K, beta = 3, 1.0
    H, W = _one_strip(orient)
    n, eid, w, lp, init = _integer_problem(5, H, W, K, False)
    w = np.zeros_like(w)
    lp = np.zeros_like(lp)
    g = M.Graph(n, eid, w)
    b = _setup(n, K, eid, w, H, W, False, lp, init)
    lab = init.astype(np.int64).copy()
    prop = M.best_alternative(g, -lp, lab, beta)
    assert np.all(prop != lab)                                   # every cell has a proposal, at a cost difference of exactly 0
    ch, ref = _run(entry, b, g, lp, lab, beta, H, W, False, orient, ONE_STRIP_CUT, K)
    assert sum(ref) == 0 and np.array_equal(lab, init)
    assert ch == 0 and np.array_equal(b.get_labels().astype(np.int64), init)
    b.close()


@pytest.mark.parametrize("entry", ["fusion", "multi"])
@pytest.mark.parametrize("H,W,diagonal", [(70, 70, True), (12, 131, False)])
def test_other_geometries_and_the_last_label(H, W, diagonal, entry):
    """(e) an upper-triangular block, a block whose last segment is short (W = 64 k + 3); K = 64 with moves to label 63."""
    K, beta = 64, 1.0
    n0 = H * (H + 1) // 2 if diagonal else H * W
    movers = np.random.default_rng(2).permutation(n0)[:n0 // 3]
    init = _integer_problem(9, H, W, K, diagonal)[4]
    movers = movers[init[movers] != 63]
    n, eid, w, lp, init, tgt = _forced_problem(9, H, W, K, diagonal, movers, targets=63)
    g = M.Graph(n, eid, w)
    b = _setup(n, K, eid, w, H, W, diagonal, lp, init)
    lab = init.astype(np.int64).copy()
    total = 0
    for orient, cut in ((0, (0, 0)), (1, (3, 17)), (0, (5, 63))):      # (nodes on a cut's fixed lines wait for the next cut)
        before = lab.copy()
        # (the launch of three labels: the model costs a second per label and pass at this size)
        ch, ref = _run(entry, b, g, lp, lab, beta, H, W, diagonal, orient, cut, K, labels=[0, 62, 63])
        moved = np.nonzero(lab != before)[0]
        assert len(moved) > 0 and np.all(lab[moved] == 63)        # precondition: this pass moves nodes, all of them to label 63
        got = b.get_labels().astype(np.int64)
        assert np.array_equal(got, lab), (orient, cut, int((got != lab).sum()))
        assert ch == sum(ref)
        total += ch
    assert total > len(movers) // 2
    b.close()


@pytest.mark.parametrize("orient", [0, 1])
def test_one_strip_moves_for_three_labels_in_one_launch(orient):
    """(f) strip_multi_pass: the strip moves for labels 1, 2 and 3 in one launch -- after each move the later labels are
    filtered again, and one wave records more than one DP run."""
    K, beta = 4, 1.0
    H, W = _one_strip(orient)
    n, eid, w, lp, init = _integer_problem(3, H, W, K, False)
    cells = np.arange(SH * SL)
    nodes_of = np.array([_cell_node(orient, W, t) for t in cells])
    pick = nodes_of[(cells % 3 == 0) & (init[nodes_of] == 0)]    # cells now at label 0, dealt over the targets 1, 2, 3
    targets = 1 + np.arange(len(pick)) % 3
    n, eid, w, lp, init, tgt = _forced_problem(3, H, W, K, False, pick, targets=targets)
    g = M.Graph(n, eid, w)
    b = _setup(n, K, eid, w, H, W, False, lp, init)
    lab = init.astype(np.int64).copy()
    ch, ref = _run("multi", b, g, lp, lab, beta, H, W, False, orient, ONE_STRIP_CUT, K)
    assert ref[0] == 0 and min(ref[1:]) > 0 and sum(ref) == len(pick)        # precondition: three labels move the one strip
    got = b.get_labels().astype(np.int64)
    assert np.array_equal(got, lab), int((got != lab).sum())
    assert ch == sum(ref)
    b.close()


def _golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strip_dp_labels.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", C.PASS_PROBLEMS, ids=[C.pass_key(*c) for c in C.PASS_PROBLEMS])
def test_pass_labels_on_real_valued_problems_are_the_recorded_ones(case):
    """fusion passes and expansions, both orientations, three cuts: the labellings hash as they did before the rework"""
    gold = _golden()
    hx, moved = C.pass_sequence_hash(*case)
    assert moved == gold["moved"][C.pass_key(*case)] and moved > 0
    assert hx == gold["hashes"][C.pass_key(*case)]


def test_solve_labels_are_the_recorded_ones(monkeypatch):
    """one cold and one warm solve_fast of a 300 x 300 upper-triangular block, K = 20, in the deterministic mode"""
    monkeypatch.setenv("PHMRF_DETERMINISTIC", "1")
    gold = _golden()["hashes"]
    cold, warm = C.solve_hashes()
    assert cold == gold["solve cold"]
    assert warm == gold["solve warm"]
