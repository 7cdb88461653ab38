"""The strip kernels (strip.hip: strip_cols_kernel, strip_kernel, propose_grid_kernel + fusion_cols_kernel) against the float64
optimum on REAL-VALUED problems, strip by strip (tests/strip_real_reference.py; tests/test_strip_real_cpu.py shows that this
check catches move models that are subtly wrong).

After every pass, with L0 the labelling before it, L1 the device's and L* that of oracle/mrf_moves.strip_fusion run from L0 on
the inputs THE BLOCK STORES (get_logprob, get_adjacency), all energies float64 and per strip:
  (i)   e_s(L1) <= e_s(L0) + a_s on every strip,
  (ii)  e_s(L1) <= e_s(L*) + a_s on every strip -- a lost or wrong move fails here,
  (iii) rim nodes never change; a changed node took alpha (expansion) or a label whose f64 proposal cost is within the
        ambiguity bound of its best alternative's (fusion),
  (iv)  the returned count is the number of changed labels.
a_s = 12 (T_s + 6) 2^-24 M_s is the f32 forward bound derived in strip_real_reference.strip_allowance.  Fusion strips that
hold a node whose two best proposals f32 cannot tell apart are left out of (ii); there may be at most 5 % of them per case.

The 'offset' family (1024 added to every unary) has an allowance of about 10 per strip, so (ii) has no teeth there: it is
in the matrix for the record of what the raw-cost accumulation of the DP loses when unaries are large, measured against
the allowance of the same problem without the offset.

The figures printed with -s (worst (e_s(L1) - e_s(L*)) / a_s and the share of strips with L1 == L* per family) are
measurements, recorded in DESIGN.md 3.1; the thresholds are (i) and (ii)."""
import collections

import numpy as np
import pytest

from oracle import mrf_moves as M
from tests import strip_real_reference as S
from tests.test_gpu_estep import _block

pytestmark = pytest.mark.gpu

FAMILY = collections.defaultdict(lambda: dict(ratio=0.0, same=0, strips=0, ratio_plain=0.0, gain=0.0, gain_model=0.0))


@pytest.fixture(scope="module", autouse=True)
def _family_record():
    yield
    for family, f in sorted(FAMILY.items()):
        line = "strip moves, %s: worst (e(L1) - e(L*)) / a_s = %.3g, L1 == L* on %d of %d strip-passes (%.2f %%)" % (
            family, f["ratio"], f["same"], f["strips"], 100.0 * f["same"] / max(f["strips"], 1))
        if family == "offset":
            line += "; against the allowance without the offset: %.3g; gain %.6g of the model's %.6g" % (
                f["ratio_plain"], f["gain"], f["gain_model"])
        print("\n" + line)


def _setup(p):
    b = _block(p.n, 4 if p.extra else 2, p.K)
    b.set_graph(p.eid, p.w)
    b.set_grid(p.H, p.W, p.diagonal, 8)
    if p.extra:
        X, means, covars = p.extra
        b.set_observations(X)
        b.emission(means, covars)
    else:
        b.set_logprob(-p.unary)
    return b


@pytest.mark.parametrize("c", S.CASES, ids=[S.case_id(c) for c in S.CASES])
def test_every_strip_reaches_the_float64_optimum(c):
    p = S.make_problem(c.family, c.seed, c.H, c.W, c.K, c.diagonal, c.beta, c.start)
    b = _setup(p)
    # the reference reads what the block stores
    un = -b.get_logprob()
    w = S.weights_from_adjacency(*b.get_adjacency(), p.eid)
    if not p.extra:
        assert np.array_equal(un, p.unary)
    assert np.array_equal(w, p.w)
    p = p._replace(unary=un, w=w)
    g = M.Graph(p.n, p.eid, p.w)
    seqs = S.sequence(c.passes, c.labels)
    beta = p.beta

    def stepper(call):
        def step(lab, orient, sr, sc, alpha):
            count = call(orient, sr, sc, alpha)
            return b.get_labels().astype(np.int64), count
        return step

    entries = [("multi", "expansion", lambda o, sr, sc, a: b.strip_multi_pass(beta, o, sr, sc, [a])),       # strip_cols_kernel
               ("single", "expansion", lambda o, sr, sc, a: b.strip_pass(beta, o, sr, sc, a)),             # strip_kernel
               ("fusion", "fusion", lambda o, sr, sc, a: b.strip_pass(beta, o, sr, sc, -1))]               # propose + fusion_cols_kernel
    memo, failures, recs = {}, [], {}
    for entry, kind, call in entries:
        b.set_labels(p.init)
        recs[entry] = S.run_sequence(p, g, seqs[kind], stepper(call), memo)
        failures += ["%s %s" % (entry, f) for r in recs[entry] for f in r.failures()]
    amb = sum(int(r.amb.sum()) for r in recs["fusion"])
    strips = sum(int((r.cells > 0).sum()) for r in recs["fusion"])
    # the whole label list in one launch ends bit-identical to the one-label launches
    b.set_labels(p.init)
    nl = len(c.labels)
    for i, (orient, (sr, sc)) in enumerate(c.passes):
        count = b.strip_multi_pass(beta, orient, sr, sc, list(c.labels))
        ones = recs["multi"][i * nl:(i + 1) * nl]
        if not np.array_equal(b.get_labels().astype(np.int64), ones[-1].L1) or count != sum(r.count for r in ones):
            failures.append("the launch of all labels on orient %d cut %s differs from the one-label launches" % (orient, (sr, sc)))
            break
    b.close()
    # the record (measurements, no thresholds)
    f = FAMILY[c.family]
    case_ratio = 0.0
    for rs in recs.values():
        for r in rs:
            case_ratio = max(case_ratio, r.excess_ratio())
            same, of = r.same_as_model()
            f["same"] += same
            f["strips"] += of
            if c.family == "offset":
                a_plain = S.strip_allowance(r.sid, p.eid, p.w, p.unary - S.OFFSET, beta, r.L0, r.prop)
                f["ratio_plain"] = max(f["ratio_plain"], r.excess_ratio(a_plain))
                f["gain"] += float((r.e0 - r.e1).sum())
                f["gain_model"] += float((r.e0 - r.es).sum())
    f["ratio"] = max(f["ratio"], case_ratio)
    print("\n%s: worst (e(L1) - e(L*)) / a_s = %.3g, ambiguous fusion strips %d of %d" % (S.case_id(c), case_ratio, amb, strips))
    assert not failures, "\n".join(failures)
    assert amb <= 0.05 * strips, (amb, strips)
    assert sum(int(r.moved.sum()) for rs in recs.values() for r in rs) > 0
