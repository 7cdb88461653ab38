"""CPU: the fixed-point audit of tests/fixed_point_audit.py (used on the GPU by tests/test_gpu_exact_skips.py) says yes to a
labelling that the move models themselves have run to their fixed point, and no once a patch of it is spoilt."""
import numpy as np

from oracle import mrf_moves as M
from oracle import ref_numpy as R
from oracle import synth
from tests import fixed_point_audit as A


def _problem(seed, H, W, K):
    rng = np.random.default_rng(seed)
    n = H * W
    X = rng.uniform(0.5, 2, (n, 2))
    e = R.grid_edges(X, H, W, False, 8)
    eid = np.int64(e[:, :2])
    w = rng.integers(1, 9, len(eid)) / 8.0
    truth = synth.label_image(rng, H, W, K, mean_run=6).reshape(-1)
    un = rng.integers(0, 12, (n, K)).astype(np.float64) * 0.5
    un[np.arange(n), truth] -= 2.0
    return M.Graph(n, eid, w), un, rng.integers(0, K, n)


def test_audit_accepts_the_models_own_fixed_point_and_reports_a_spoilt_patch():
    H = W = 40
    K, beta = 4, 1.0
    g, un, init = _problem(3, H, W, K)
    n = H * W
    col, nc = M.icm_colours(H, W, False)
    sr, sc = A.GEOM_R[0], A.GEOM_C[0]
    fr, fc = (sr + A.FUSION_SHIFT[0]) % 6, (sc + A.FUSION_SHIFT[1]) % 64
    lab = init.astype(np.int64).copy()
    # the random start is no fixed point, on any cut
    assert A.fixed_cuts(A.audit(g, un, lab, beta, H, W, False, first_move_only=True)) == []
    for sweep in range(50):                   # every move type of a verification round on cut 0, until a whole round is quiet
        ch = M.component_pass(g, un, lab, beta)
        for family in range(4):
            ch += A.segment_chain_model(g, un, lab, beta, H, W, False, family, 1)
        ch += M.icm_sweep(g, un, lab, beta, col, nc)
        for orient in (0, 1):
            ch += M.strip_fusion(g, un, lab, M.best_alternative(g, un, lab, beta), beta, H, W, False, orient, fr, fc)
            for alpha in range(K):
                ch += M.strip_fusion(g, un, lab, np.full(n, alpha), beta, H, W, False, orient, sr, sc)
        if ch == 0:
            break
    assert ch == 0 and sweep >= 1
    report = A.audit(g, un, lab, beta, H, W, False, cuts=(0,))
    assert 0 in A.fixed_cuts(report), [p for p in report[0] if p[1]]
    # every move type was asked: component, four chain families, ICM, two fusion passes, K expansions per orientation
    assert len(report[0]) == 1 + 4 + 1 + 2 + 2 * K
    # a 6 x 6 patch flipped to its second-best label: some move takes it back, on every cut
    second = M.best_alternative(g, un, lab, beta).reshape(H, W)
    bad = lab.reshape(H, W).copy()
    bad[17:23, 9:15] = second[17:23, 9:15]
    bad = bad.reshape(-1)
    assert M.energy(g, un, bad, beta)[0] > M.energy(g, un, lab, beta)[0]
    full = A.audit(g, un, bad, beta, H, W, False)
    assert A.fixed_cuts(full) == [], full
    assert all(sum(ch for _, ch in pairs) > 0 for pairs in full.values())
    short = A.audit(g, un, bad, beta, H, W, False, first_move_only=True)
    assert A.fixed_cuts(short) == []
