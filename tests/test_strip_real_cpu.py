"""CPU: the per-strip check of tests/test_gpu_strip_real.py can fail.  On every case of the GPU matrix (but the 'offset'
family, whose allowance is too large to catch anything) the float64 move model passes the check with no allowance at all,
three move models that are wrong on purpose (tests/strip_real_reference.MUTANTS) each miss a strip's optimum by more than
the allowance, and most strips that move gain more than ten times the allowance.  The seeds of the matrix are fixed so
that all of this holds."""
import numpy as np
import pytest

from oracle import mrf_moves as M
from tests import strip_real_reference as S

CPU_CASES = [c for c in S.CASES if c.family != "offset"]
ENTRIES = ("expansion", "fusion")


def _model_records(c):
    p = S.make_problem(c.family, c.seed, c.H, c.W, c.K, c.diagonal, c.beta, c.start)
    g = M.Graph(p.n, p.eid, p.w)
    seqs = S.sequence(c.passes, c.labels)
    memo = {}

    def step(lab, orient, sr, sc, alpha):
        key = (orient, sr, sc, alpha, lab.tobytes())
        memo[key] = S.model_pass(p, g, lab, orient, sr, sc, alpha)
        return memo[key], None

    return p, g, {e: S.run_sequence(p, g, seqs[e], step, memo) for e in ENTRIES}


@pytest.mark.parametrize("c", CPU_CASES, ids=[S.case_id(c) for c in CPU_CASES])
def test_the_check_passes_the_model_and_catches_the_mutants(c):
    p, g, recs = _model_records(c)
    every = [r for e in ENTRIES for r in recs[e]]
    # the model holds (i) .. (iii) with allowance 0 ((ii) compares it with itself; (i) says the exact move never costs)
    assert [f for r in every for f in r.failures(scale=0.0)] == []
    # the check is sharp: at least half of the strip-passes that move gain more than ten allowances
    moved = sharp = 0
    for r in every:
        gain = r.e0 - r.es
        moved += int((gain > 0).sum())
        sharp += int((gain > 10 * r.a).sum())
    assert moved > 0 and 2 * sharp >= moved, (moved, sharp)
    # fusion: at most 5 % of the strips hold a node whose best two proposals f32 cannot tell apart (they are left out of (ii))
    amb = sum(int(r.amb.sum()) for r in recs["fusion"])
    strips = sum(int((r.cells > 0).sum()) for r in recs["fusion"])
    assert amb <= 0.05 * strips, (amb, strips)
    # each mutant, run on the labellings the model passes through, misses the optimum of a strip by more than the allowance
    # (the passes are tried in turn up to the first one that shows it)
    for name, mutant in S.MUTANTS.items():
        misses = 0
        for r in every:
            L1 = mutant(p, g, r.L0, r.orient, r.cut[0], r.cut[1], r.alpha)
            check = S.PassCheck(p, g, r.L0, L1, r.orient, r.cut[0], r.cut[1], r.alpha, r.Ls)
            misses = check.misses()
            if misses:
                assert any(f.startswith("(ii)") for f in check.failures())
                break
        assert misses > 0, name


def test_the_matrix_is_the_stated_one():
    """the shapes, label counts, betas, cuts, orientations, families and starts the GPU test is to cover"""
    shapes = {(c.H, c.W, c.diagonal) for c in S.CASES}
    assert shapes == {(12, 20, False), (23, 70, False), (12, 131, False), (7, 64, False), (41, 41, True), (64, 64, True),
                      (12, 40, False)}
    assert {(c.H, c.W, c.diagonal) for c in S.CASES if c.family == "real"} == shapes
    assert {c.K for c in S.CASES} == {4, 8, 20, 64} and {c.beta for c in S.CASES} == {0.5, 0.75, 2.0}
    k64 = [c for c in S.CASES if c.K == 64]
    assert len(k64) == 1 and (k64[0].H, k64[0].W) == (12, 40) and len(k64[0].labels) == 8 and 63 in k64[0].labels
    assert {(o, cut) for c in S.CASES for o, cut in c.passes} == {(o, cut) for o in (0, 1) for cut in ((0, 0), (3, 17), (5, 63))}
    for family in ("emission", "offset"):
        assert len({(c.H, c.W) for c in S.CASES if c.family == family}) == 2
    assert sum(c.start == "random" for c in S.CASES) == 2


def test_strip_quantities_on_a_hand_made_strip():
    """strip_ids, strip_energies and strip_allowance on a 7 x 10 block whose one strip with cells on the cut (5, 63) is rows
    1 .. 5 of columns 1 .. 9 (strip 1: the band above it lies outside the block): every figure counted by hand"""
    H, W = 7, 10
    sid = S.strip_ids(H, W, False, 0, 5, 63)
    grid = sid.reshape(H, W)
    assert np.all(grid[1:6, 1:] == 1) and np.all(grid[0] == -1) and np.all(grid[6] == -1) and np.all(grid[:, 0] == -1)
    eid = np.array([[11, 12], [1, 11], [11, 21], [0, 1], [12, 21]])          # inside, rim-strip, inside, rim-rim, anti-diagonal inside
    w = np.array([0.5, 0.25, 1.0, 8.0, 2.0])
    un = np.zeros((H * W, 2))
    un[11] = [3.0, -7.0]
    un[12] = [1.0, 2.0]
    lab = np.zeros(H * W, dtype=np.int64)
    lab[11] = 1
    e = S.strip_energies(sid, eid, w, un, 2.0, lab)
    assert e.shape == (2,) and e[0] == 0.0 and e[1] == (-7.0 + 1.0) + 2.0 * (0.5 + 0.25 + 1.0)
    a = S.strip_allowance(sid, eid, w, un, 2.0, lab, 1 - lab)
    Ms = (7.0 + 2.0 * 1.75) + (2.0 + 2.0 * 2.5) + 2.0 * 3.0          # nodes 11, 12, 21 (the others: no unary, no edge)
    assert a[0] == 0.0 and a[1] == 12 * (45 + 6) * 2.0 ** -24 * Ms
    with pytest.raises(AssertionError):                                  # an edge between two strips is a broken geometry
        S.strip_energies(np.array([0, 1]), np.array([[0, 1]]), np.ones(1), np.zeros((2, 2)), 1.0, np.zeros(2, dtype=np.int64))


def test_ambiguous_proposals_are_those_f32_cannot_tell_apart():
    eid = np.array([[0, 1], [1, 2]])
    g = M.Graph(3, eid, np.array([1.0, 1.0]))
    un = np.array([[0.0, 5.0, 5.0 + 1e-7, 9.0], [0.0, 5.0, 5.1, 9.0], [0.0, 1.0, 2.0, 3.0]])
    lab = np.zeros(3, dtype=np.int64)
    amb = S.ambiguous_proposals(g, un, lab, 1.0)
    assert amb.tolist() == [True, False, False]           # 1e-7 < 8 * 2^-24 * (5 + 5 + 1) = 5.2e-6 < 0.1
    assert M.best_alternative(g, un, lab, 1.0).tolist() == [1, 1, 1]
