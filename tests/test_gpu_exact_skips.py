"""GPU (run with -m gpu on an MI355X): what the label solver claims about its own shortcuts and its own stopping rule.

1. The exact skips ("Skipping work exactly") change no labelling.  Every label write stamps the node and its
   neighbours with the launch tick; strips (strip.hip) and chain segments (moves.hip) keep the tick of their last quiet run
   and are skipped while no newer stamp lies on their cells; proposals are recomputed only in waves that carry a newer
   stamp; row tiles stamp the halo rows they receive.  With PHMRF_NO_SKIP (development library only) the memos are not
   passed and every proposal is recomputed, the stamps are still written and nothing else changes: cold and warm solves
   must then walk through the same labellings, bit for bit, as the product library does with its skips.
2. `converged` means a fixed point of the move models (tests/fixed_point_audit.py), on exactly representable problems.

The single-pass entry points that tests/test_gpu_estep.py compares with the models run outside a solve (tick 0, no named
cut): no stamp is written, no memo is read and no proposal tile is skipped in any of them.  These tests are the ones that
hold the stamped, memoised paths of a solve to something stricter than "the energy went down"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import mrf_moves as M
from tests import fixed_point_audit as A
from tests.test_gpu_estep import _block, _integer_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (H, W, diagonal, K, num_neighbor, energy_tol_ppb, extra solve options, row tiles)
SKIP_CASES = {
    "tri500_k12_tol0": (500, 500, True, 12, 8, 0, {}, 0),
    "tri500_k12_tol1000": (500, 500, True, 12, 8, 1000, {}, 0),
    "tri500_k12_tol10000": (500, 500, True, 12, 8, 10000, {}, 0),
    "rect300x420_k12": (300, 420, False, 12, 8, 10000, {}, 0),          # orientation 1 differs; W is no multiple of 64
    "rect130x193_k64": (130, 193, False, 64, 8, 1000, {}, 0),           # 64 label ticks per launch, full masks
    "rect257x70_k5_nn4": (257, 70, False, 5, 4, 1000, {}, 0),           # the 4-stencil's own dilation pattern
    "tri500_k12_no_expansion": (500, 500, True, 12, 8, 1000, {"use_expansion": False}, 0),   # chain memo live from round 2
    "tri500_k12_three_tiles": (500, 500, True, 12, 8, 1000, {}, 3),     # halo rows arrive from outside the tile
    # the one case at or above 2^18 nodes, where the product takes the incremental energy from the second round on: here the
    # arm with PHMRF_ENERGY_FULL differs from the product arm in fact (every smaller block takes the full pass in both)
    "rect513x513_k5": (513, 513, False, 5, 8, 1000, {}, 0),
}

SKIP_SCRIPT = r"""
import os, sys, hashlib
import numpy as np
sys.path.insert(0, os.environ["PHMRF_ROOT"])
import torch
from phylo_hmrf_amd import Block, synthetic, tiles
from phylo_hmrf_amd.tree import PhyloTree
CASES = @CASES@
S = 4
dev = torch.device("cuda", 0)

def emissions(K):            # the data's own parameters, then 15 % off them, then 5 % off those
    tree = PhyloTree(synthetic.tree_for(S)); rng = np.random.default_rng(4)
    P = synthetic.sample_ou_params(rng, tree, K)
    P2 = np.clip(P * (1 + 0.15 * rng.standard_normal(P.shape)), 1e-3, 50)
    P3 = np.clip(P2 * (1 + 0.05 * rng.standard_normal(P.shape)), 1e-3, 50)
    out = []
    for q in (P, P2, P3):
        mu, cv = tree.mean_cov(q)
        out.append((mu, cv + 1e-3 * np.eye(S)))
    return out

def sha(lab):
    return hashlib.sha1(np.ascontiguousarray(lab, dtype=np.int32).tobytes()).hexdigest()

for name, (H, W, diag, K, nn, tol, extra, parts) in CASES.items():
    em = emissions(K)
    X = synthetic.device_observations(torch, dev, 10, H, W, diag, K, *em[0]); torch.cuda.synchronize()
    n = H * (H + 1) // 2 if diag else H * W
    out = []
    if not parts:
        b = Block(n, S, K); b.set_observations_dev(X.data_ptr()); b.sync(); b.build_grid_graph(H, W, diag, nn, 0.5)
        b.enable_timing(True, classes=[])              # (the work counters, no event pairs)
        for i, (mu, cv) in enumerate(em):
            b.emission(mu, cv); b.reset_timing()
            res = b.solve(1.0, energy_tol_ppb=tol, init_mode=1 if i == 0 else 0, **extra)
            w = b.work()
            out.append((sha(b.get_labels()), res["rounds"], res["changed"], repr(res["energy"]), w["units"], w["proposal_nodes"],
                        b.incremental_energies()))
        b.close()
    else:
        Xh = X.cpu().numpy().astype(np.float64)
        rows = tiles.split_rows(H, W, diag, parts)
        def load(tl):
            tl.b.set_observations(Xh[tl.global_slice()])
        g = tiles.make_group(0, (H, W, diag), rows, [0] * parts, 0, S, K, Block, load, None, nn, 0.5)
        for tl in g.local.values():
            tl.b.enable_timing(True, classes=[])
        for i, (mu, cv) in enumerate(em[:2]):
            for tl in g.local.values():
                tl.b.emission(mu, cv); tl.b.reset_timing()
            g.begin(1.0, dict(energy_tol_ppb=tol, init_mode=1 if i == 0 else 0, **extra))
            while True:
                g.launch()
                if g.finish_round() != 0:
                    break
            res = g.end(want_result=True)
            lab = np.zeros(n, dtype=np.int32)
            for tl in g.local.values():
                lab[tl.owned_global_slice()] = tl.b.get_labels()[tl.owned_local_slice()]
            w = [tl.b.work() for tl in g.local.values()]
            out.append((sha(lab), res["rounds"], res["changed"], repr(res["energy"]), sum(x["units"] for x in w),
                        sum(x["proposal_nodes"] for x in w), sum(tl.b.incremental_energies() for tl in g.local.values())))
        for tl in g.local.values():
            tl.b.close()
    del X
    print("RESULT", repr(name), out, flush=True)
"""


@pytest.fixture(scope="module")
def skip_arms():
    """Both arms, one child process each (PHMRF_DETERMINISTIC=1): the product library with its skips, and the development
    library with PHMRF_NO_SKIP and PHMRF_ENERGY_FULL (the incremental energy is a skip of its own kind, with its own knob).
    -> {arm: {case: [(label sha1, rounds, changed, repr(energy), units, proposal_nodes, incremental energy evaluations) per
    solve]}}"""
    dev = os.path.join(ROOT, "phylo_hmrf_amd", "libphmrf_dev.so")      # (the knobs exist in the -DPHMRF_DEV build only)
    assert os.path.exists(dev), "libphmrf_dev.so not built (make -C phylo_hmrf_amd/csrc)"
    script = SKIP_SCRIPT.replace("@CASES@", repr(SKIP_CASES))
    arms = {}
    for arm, extra in (("skips", {}), ("no skips", {"PHMRF_LIB": dev, "PHMRF_NO_SKIP": "1", "PHMRF_ENERGY_FULL": "1"})):
        env = dict(os.environ, PHMRF_ROOT=ROOT, PHMRF_DETERMINISTIC="1", **extra)
        if arm == "skips":
            for k in ("PHMRF_LIB", "PHMRF_NO_SKIP", "PHMRF_ENERGY_FULL"):
                env.pop(k, None)
        out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=1200, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        res = {}
        for ln in out.stdout.splitlines():
            if ln.startswith("RESULT"):
                name, runs = eval("(" + ln[len("RESULT"):].strip().replace(" ", ",", 1) + ")")
                res[name] = runs
        arms[arm] = res
    return arms


@pytest.mark.parametrize("case", sorted(SKIP_CASES))
def test_exact_skips_leave_every_labelling_alone(skip_arms, case):
    """A cold solve and the warm solves after new emissions give, solve for solve, the same label hash, round count, number
    of changed labels and energy with the memos and the proposal skip (product library) and without them (PHMRF_NO_SKIP).
    Teeth: in every warm solve the arm with the skips stages strictly fewer strips and computes strictly fewer proposals
    than the arm without, so the knob took effect and the skips were exercised; every cold solve runs at least three
    rounds, every warm solve at least two.  The incremental energy (energy_round_launch: blocks of 2^18 nodes and more, from
    a solve's second evaluation on) ran in every solve of such a block in the product arm and in none with
    PHMRF_ENERGY_FULL; smaller blocks never take it.

    Measured on an MI355X (both arms equal in every entry; rounds per solve | strips staged, with skips : without |
    proposals computed, with : without; the test prints them, -s):
      tri500_k12_tol0          9, 8, 8 | 46733, 37377, 34476 : 73930, 53758, 60172 | 360130, 256900, 203458 : 1878750, 1753500, 1503000
      tri500_k12_tol1000       5, 4, 3 | 38690, 23028, 13287 : 55224, 30402, 23691 | 358338, 254724, 200514 : 1252500, 1002000, 626250
      tri500_k12_tol10000      5, 3, 2 | 38690, 22966, 13021 : 54379, 27028, 20780 | 358338, 254276, 200514 : 1252500, 751500, 501000
      rect300x420_k12          4, 3, 3 | 36445, 14716, 20973 : 47164, 23166, 25371 | 339536, 253248, 214112 : 1008000, 630000, 630000
      rect130x193_k64          6, 6, 3 | 50535, 30522, 17345 : 63534, 43814, 22992 | 87878, 68418, 51842 : 275990, 275990, 125450
      rect257x70_k5_nn4        3, 3, 2 | 1873, 1379, 1116 : 2759, 2040, 1672 | 35974, 37190, 33862 : 107940, 89950, 71960
      tri500_k12_no_expansion  6, 7, 3 | 1746, 964, 979 : 4217, 3429, 2535 | 197506, 163586, 155266 : 1252500, 1127250, 751500
      tri500_k12_three_tiles   7, 6 | 50322, 43181 : 69330, 54533 | 379234, 271665 : 1519728, 1266440
    """
    fast, slow = skip_arms["skips"][case], skip_arms["no skips"][case]
    n_solves = 2 if SKIP_CASES[case][7] else 3
    print("\n%s: rounds %s  units %s : %s  proposal_nodes %s : %s" % (case, [r[1] for r in fast], [r[4] for r in fast],
                                                                     [r[4] for r in slow], [r[5] for r in fast], [r[5] for r in slow]))
    assert len(fast) == len(slow) == n_solves
    for i, (f, s) in enumerate(zip(fast, slow)):
        assert f[:4] == s[:4], ("solve %d" % i, f, s)
    assert fast[0][1] >= 3, fast
    for i in range(1, n_solves):
        assert fast[i][1] >= 2, fast
        assert fast[i][4] < slow[i][4], ("units, warm solve %d" % i, fast[i], slow[i])
        assert fast[i][5] < slow[i][5], ("proposal_nodes, warm solve %d" % i, fast[i], slow[i])
    H, W, diag, parts = SKIP_CASES[case][0], SKIP_CASES[case][1], SKIP_CASES[case][2], SKIP_CASES[case][7]
    large = not parts and (H * (H + 1) // 2 if diag else H * W) >= 1 << 18
    for f, s in zip(fast, slow):
        assert s[6] == 0, ("incremental energy evaluations with PHMRF_ENERGY_FULL", s)
        assert (f[6] > 0) if large else (f[6] == 0), ("incremental energy evaluations", f)


# ------------------------------------------------------------------------------------------------ converged = fixed point
# (measured: 7, 5, 9, 7 and 4 rounds; each result is a fixed point on all three cuts; no case is coarse-only)
FIXED_POINT_CASES = [(4, 41, 41, 6, True, 1.0), (6, 64, 129, 20, False, 0.5), (11, 30, 66, 64, False, 2.0),
                     (4, 130, 7, 5, False, 1.0), (6, 70, 70, 12, True, 0.5)]
_coarse_only_cases = []    # cases whose last changing round moved labels at the coarse scales alone (at most one may)


def _solve_in_pieces(b, beta):
    """an exact solve from the block's labels, round by round -> (status, [(labels after the round, its counters)])"""
    b.solve_begin(beta, energy_tol_ppb=0, init_mode=0, max_rounds=4000)     # (the tick budget of solve.hip still bounds it)
    rounds = []
    while True:
        b.solve_round_launch()
        c, e = b.solve_round_collect()
        st = b.solve_round_decide(c, e)
        rounds.append((b.get_labels().astype(np.int64), c.copy()))
        if st != 0:
            break
    res = b.solve_end(want_result=True)
    return st, res, rounds


@pytest.mark.parametrize("seed,H,W,K,diagonal,beta", FIXED_POINT_CASES)
def test_converged_is_a_fixed_point_of_the_move_models(seed, H, W, K, diagonal, beta):
    """Dyadic inputs (f32 arithmetic is exact), the product library, an exact solve (tolerance 0) from random labels.
    (1) the solve reports `converged` and its last round changed nothing; (2) on at least one of the three fixed cuts no
    move model moves a label of the final labelling: every label's strip expansion and the fusion with the best
    alternatives in both orientations, the component pass, the four chain families at the verification round's segment
    cut, ICM (the coarse expansions are left out, see tests/fixed_point_audit.py); (3) nor do the GPU's own memo-free single
    passes on that cut, on a second block; (4) the audit can say no: the random start is no fixed point on any cut, and the
    labelling before the last round that changed labels is none on at least one.

    (3), chain moves: phmrf_mrf_chain_sweep runs BOTH segment cuts of a family, the verification round only the second.
    Where the model's first cut moves nothing either the GPU sweep must report 0; otherwise it must end at the model's
    energy (the assertion of test_chain_sweeps_match_move_model)."""
    from phylo_hmrf_amd import _lib
    slots = slice(_lib.COUNTER_EXPANSION, _lib.COUNTER_COARSE + 3)
    coarse = slice(_lib.COUNTER_COARSE, _lib.COUNTER_COARSE + 3)
    n, eid, w, lp, init = _integer_problem(seed, H, W, K, diagonal)
    g, un = M.Graph(n, eid, w), -lp
    init = init.astype(np.int64)
    b = _block(n, 2, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 8)
    b.set_logprob(lp)
    b.set_labels(init)
    st, res, rounds = _solve_in_pieces(b, beta)
    b.close()
    assert st == 1 and res["converged"], (st, res)
    assert int(rounds[-1][1][slots].sum()) == 0 and res["rounds"] == len(rounds)
    L = rounds[-1][0]
    e_L = M.energy(g, un, L, beta)[0]
    assert res["energy"] == e_L                              # exact arithmetic: no tolerance
    # (2) the models
    report = A.audit(g, un, L, beta, H, W, diagonal, first_move_only=True)
    fixed = A.fixed_cuts(report)
    print("\n%d x %d K %d beta %g: %d rounds, fixed point on cut(s) %s" % (H, W, K, beta, len(rounds), fixed))
    assert fixed, dict((c, [p for p in pairs if p[1]]) for c, pairs in report.items())
    cut = fixed[0]
    assert len(report[cut]) == 6 + 2 + 2 * K                # every move type was asked
    # (3) the GPU's single passes, each on the labelling L itself
    b2 = _block(n, 2, K)
    b2.set_graph(eid, w)
    b2.set_grid(H, W, diagonal, 8)
    b2.set_logprob(lp)
    sr, sc = A.GEOM_R[cut], A.GEOM_C[cut]
    fr, fc = (sr + A.FUSION_SHIFT[0]) % 6, (sc + A.FUSION_SHIFT[1]) % 64
    passes = [("expansions orient %d" % o, lambda o=o: b2.strip_multi_pass(beta, o, sr, sc)) for o in (0, 1)]
    passes += [("fusion orient %d" % o, lambda o=o: b2.strip_pass(beta, o, fr, fc, -1)) for o in (0, 1)]
    passes += [("component", lambda: b2.component_pass(beta)), ("icm", lambda: b2.icm_sweep(beta))]
    for name, run in passes:
        b2.set_labels(L)
        assert run() == 0, name
        assert np.array_equal(b2.get_labels(), L), name
    for family in range(4):
        b2.set_labels(L)
        ch = b2.chain_sweep(beta, family)
        ref = L.copy()
        ch0 = A.segment_chain_model(g, un, ref, beta, H, W, diagonal, family, 0)
        A.segment_chain_model(g, un, ref, beta, H, W, diagonal, family, 1)
        if ch0 == 0:
            assert ch == 0 and np.array_equal(b2.get_labels(), L), ("chain family", family, ch)
        else:
            assert abs(M.energy(g, un, b2.get_labels().astype(np.int64), beta)[0] - M.energy(g, un, ref, beta)[0]) < 1e-9
    b2.close()
    # (4) teeth
    assert A.fixed_cuts(A.audit(g, un, init, beta, H, W, diagonal, first_move_only=True)) == []
    last = max(i for i, (_, c) in enumerate(rounds) if int(c[slots].sum()) > 0)
    counters = rounds[last][1]
    before = rounds[last - 1][0] if last > 0 else init
    if int(counters[slots].sum()) == int(counters[coarse].sum()):
        _coarse_only_cases.append((seed, H, W, K, diagonal, beta))      # the audit leaves the coarse moves out
        assert len(_coarse_only_cases) <= 1, _coarse_only_cases
    else:
        rep = A.audit(g, un, before, beta, H, W, diagonal, first_move_only=True)
        assert len(A.fixed_cuts(rep)) < 3, "the labelling before the last changing round passes as a fixed point on every cut"
