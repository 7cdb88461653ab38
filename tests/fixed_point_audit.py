"""TEST INFRASTRUCTURE ONLY -- is a labelling a fixed point of the solver's move types, by the float64 move models?

`phmrf_solve_result.converged == 1` is documented as "ended at a fixed point of all move types" (include/phmrf.h).  A
solve ends after a quiet VERIFICATION round: every move type active, chain segments cut at their second set of separators
(phase 1), the strip expansions on one of three fixed cuts and the strip fusion on that cut shifted by half a band and
half a segment.  The audit below replays that round with the models of oracle/mrf_moves.py, every move on a copy of the
labelling of its own.  The coarse expansions are left out: their child cuts depend on the round number (round_coarse in
solve.hip), which the boundary does not report; a fixed point of the other move types must hold whether or not they ran.

Pure NumPy: tests/test_fixed_point_audit.py checks the audit itself without a GPU."""
import numpy as np

from oracle import mrf_moves as M

# the three fixed cuts of the strip expansions and the fusion pass's shift against them: csrc/solve.hip (GEOM_R, GEOM_C,
# and round_strips: (GEOM_R[g] + 3) % 6, (GEOM_C[g] + 31) % 64)
GEOM_R = (0, 2, 4)
GEOM_C = (0, 21, 42)
FUSION_SHIFT = (3, 31)


def segment_chain_model(g, un, labels, beta, H, W, diagonal, family, phase):
    """oracle/mrf_moves chain move restricted to the product's segment cut (<=63 nodes, separators fixed)."""
    fam = M.chain_families(H, W, diagonal, 8)[family]
    chains, colour, ncol = fam
    changed = 0
    for c in range(ncol):
        segs = []
        for ch, cc in zip(chains, colour):
            if cc != c:
                continue
            L = len(ch)
            start, sep = 0, (31 if phase else 63)
            while start < L:
                end = min(sep, L)
                if end > start:
                    segs.append(ch[start:end])
                start = sep + 1
                sep += 64
        if not segs:
            continue
        nodes, lens, col2, _ = M.pack_family((segs, np.zeros(len(segs), dtype=np.int64), 1))
        changed += M.chain_move(g, un, labels, beta, nodes, lens, np.ones(len(segs), dtype=bool))
    return changed


def _on_copy(labels, move):
    lab = labels.copy()
    ch = int(move(lab))
    assert ch == int((lab != labels).sum()), "a move model miscounts its own changes"
    return ch


def cut_free_moves(graph, unary, labels, beta, H, W, diagonal):
    """The move types that do not depend on the strip cut -> [(move type, labels changed)]."""
    labels = np.asarray(labels, dtype=np.int64)
    out = [("component", _on_copy(labels, lambda l: M.component_pass(graph, unary, l, beta)))]
    for family in range(4):
        out.append(("chain family %d phase 1" % family,
                    _on_copy(labels, lambda l: segment_chain_model(graph, unary, l, beta, H, W, diagonal, family, 1))))
    col, nc = M.icm_colours(H, W, diagonal)
    out.append(("icm", _on_copy(labels, lambda l: M.icm_sweep(graph, unary, l, beta, col, nc))))
    return out


def cut_moves(graph, unary, labels, beta, H, W, diagonal, g, first_move_only=False):
    """The strip moves of cut g: every label's expansion and the fusion with the best alternatives, both orientations
    -> [(move type, labels changed)].  first_move_only: stop at the first move that changes a label."""
    labels = np.asarray(labels, dtype=np.int64)
    n, K = unary.shape
    sr, sc = GEOM_R[g], GEOM_C[g]
    fr, fc = (sr + FUSION_SHIFT[0]) % 6, (sc + FUSION_SHIFT[1]) % 64
    prop = M.best_alternative(graph, unary, labels, beta)
    out = []
    for orient in (0, 1):
        out.append(("fusion orient %d" % orient,
                    _on_copy(labels, lambda l: M.strip_fusion(graph, unary, l, prop, beta, H, W, diagonal, orient, fr, fc))))
        if first_move_only and out[-1][1]:
            return out
    for orient in (0, 1):
        for alpha in range(K):
            out.append(("expansion %d orient %d" % (alpha, orient),
                        _on_copy(labels, lambda l: M.strip_fusion(graph, unary, l, np.full(n, alpha), beta, H, W, diagonal,
                                                                  orient, sr, sc))))
            if first_move_only and out[-1][1]:
                return out
    return out


def audit(graph, unary, labels, beta, H, W, diagonal, cuts=(0, 1, 2), first_move_only=False):
    """-> {cut g: [(move type, labels changed), ...]}: what every move type of a verification round on cut g does to
    `labels` (each on a copy of its own).  The labelling is a fixed point on cut g iff every count is 0 (fixed_cuts).
    first_move_only: a cut's list ends with the first move found (enough to say "not a fixed point", much cheaper)."""
    free = cut_free_moves(graph, unary, labels, beta, H, W, diagonal)
    moved = any(ch for _, ch in free)
    out = {}
    for g in cuts:
        if first_move_only and moved:
            out[g] = list(free)
        else:
            out[g] = list(free) + cut_moves(graph, unary, labels, beta, H, W, diagonal, g, first_move_only)
    return out


def fixed_cuts(report):
    """the cuts of an audit's report on which nothing moved"""
    return [g for g, pairs in sorted(report.items()) if all(ch == 0 for _, ch in pairs)]
