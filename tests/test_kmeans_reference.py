"""tests/kmeans_reference.py on the CPU: the model against brute force, the exactness claim of the dyadic cases, the tie
cap of the real-valued cases, and the bounds against a float32 emulation of the kernel's scheme (they hold for it and
fail for a dropped node).  tests/test_gpu_kmeans.py holds the device to the same model, cases and bounds."""
import numpy as np
import pytest

from oracle import ref_numpy as R
from tests import kmeans_reference as KR

IDS = [KR.case_id(c) for c in KR.CASES]
DYADIC = [c for c in KR.CASES if c[4] == "dyadic"]
REAL = [c for c in KR.CASES if c[4] == "real"]


def _brute(X, C, own):
    n, S = X.shape
    K = C.shape[0]
    lab = np.zeros(n, dtype=np.int64)
    counts, sums, outer, inertia = np.zeros(K), np.zeros((K, S)), np.zeros((K, S, S)), 0.0
    for i in range(n):
        best, bk = None, 0
        for k in range(K):
            d = sum((X[i, s] - C[k, s]) ** 2 for s in range(S))
            if best is None or d < best:
                best, bk = d, k
        lab[i] = bk
        if own[0] <= i < own[1]:
            counts[bk] += 1
            sums[bk] += X[i]
            outer[bk] += np.outer(X[i], X[i])
            inertia += best
    return lab, counts, sums, outer, inertia


@pytest.mark.parametrize("n,S,K,own", [(1, 1, 1, None), (7, 2, 3, None), (40, 3, 5, (7, 29)), (40, 4, 5, (0, 0)), (33, 2, 4, (32, 33)),
                                       (25, 5, 6, (0, 24))])
def test_model_against_brute_force(n, S, K, own):
    """integer-valued inputs (every sum exact, many ties), own ranges including an empty and a one-node one, and a centre far
    from every node (an empty cluster) next to a duplicated one"""
    rng = np.random.default_rng(n + S + K)
    X = rng.integers(0, 4, (n, S)).astype(np.float64)
    C = rng.integers(0, 4, (K, S)).astype(np.float64)
    if K >= 3:
        C[1] = 50.0                                    # no node is nearest to it
        C[K - 1] = C[0]                                # never wins the tie
    want = _brute(X, C, own if own else (0, n))
    got = KR.step(X, C, own)
    assert np.array_equal(got[0], want[0])
    assert all(np.array_equal(g, w) for g, w in zip(got[1:4], want[1:4])) and got[4] == want[4]
    if K >= 3:
        assert got[1][1] == 0 and got[1][K - 1] == 0
    if own is None:                                    # the part the oracle's own step covers
        lab, sums, counts, inertia = R.kmeans_step(X, C)
        assert np.array_equal(lab, got[0]) and np.array_equal(sums, got[2]) and np.array_equal(counts, got[1]) and inertia == got[4]


def test_the_case_list_covers_what_it_claims():
    forms = {(c[0], c[1]) for c in KR.FORM_CASES if c[4] == "dyadic"} & {(c[0], c[1]) for c in KR.FORM_CASES if c[4] == "real"}
    assert forms == {("step", S) for S in range(1, 17)} | {("moments", S) for S in range(1, 9)}
    for entry in ("step", "moments"):
        assert {c[2] for c in KR.FORM_CASES if c[0] == entry} == set(KR.KSET)
    assert ("moments", 8, 64) in {c[:3] for c in KR.FORM_CASES}
    assert {(c[0], c[1], c[3]) for c in KR.EDGE_CASES} == {(e, S, n) for e in ("step", "moments") for S in (3, 4)
                                                          for n in (1, 255, 256, 257, 511, 513)}
    assert KR.TRIP_N == 2048 * 256 + 300 and {c[:2] for c in KR.TRIP_CASES} == {(e, S) for e in ("step", "moments") for S in (3, 4)}
    assert len(set(IDS)) == len(IDS)
    # the sizes the API admits: 8 + K*S + K + 1 + K*S*S doubles of the accumulator area (8192)
    assert all(8 + K * S + K + 1 + (K * S * S if e == "moments" else 0) <= 8192 for e, S, K, _, _ in KR.CASES)


@pytest.mark.parametrize("c", DYADIC, ids=[KR.case_id(c) for c in DYADIC])
def test_dyadic_cases_are_exact_in_float32_and_hold_ties(c):
    """the float32 emulation (shuffled tile order) equals the float64 model bit for bit, and the case has exact ties at the
    minimum that "highest index wins" would decide differently"""
    case = KR.case(*c)
    assert np.array_equal(case.X * 8, np.round(case.X * 8)) and case.X.min() >= 0 and case.X.max() < 4
    assert np.array_equal(case.C * 8, np.round(case.C * 8)) and case.C.min() >= 0 and case.C.max() < 4
    KR.check_exact(case.X, case.C, KR.emulate(case.X, case.C, rng=np.random.default_rng(1)))
    if case.n > 300:                                  # a tile with its own range, as a row tile has
        own = (case.n // 7, case.n - 100)
        KR.check_exact(case.X, case.C, KR.emulate(case.X, case.C, own=own, rng=np.random.default_rng(2)), own=own)
    if case.K >= 2:
        lab, d1, d2 = KR.two_smallest(case.X, case.C)
        assert np.count_nonzero(d1 == d2) >= 1
        # the planted midway nodes: centres 0 and 1 tie at THEIR minimum (1/64 each, no third centre closer), centre 0 wins
        mid = KR.midway_nodes(case.X, case.C)
        dm = ((case.X[mid, None, :] - case.C[None, :, :]) ** 2).sum(axis=2)
        won = (dm[:, 0] == dm.min(axis=1)) & (dm[:, 1] == dm[:, 0]) & (dm[:, 0] == 1.0 / 64.0)
        assert mid.size >= 1 and np.count_nonzero(won) >= 1 and np.all(lab[mid[won]] == 0)
        if case.K >= 3:
            assert np.bincount(lab, minlength=case.K)[case.K - 1] == 0          # the duplicate's cluster is empty


@pytest.mark.parametrize("c", REAL, ids=[KR.case_id(c) for c in REAL])
def test_real_cases_keep_the_tie_cap_and_their_bounds_bite(c):
    case = KR.case(*c)
    assert np.array_equal(case.X, KR.f32(case.X)) and np.array_equal(case.C, KR.f32(case.C))
    assert KR.near_ties(case.X, case.C).size <= KR.tie_cap(case.n)
    got = KR.emulate(case.X, case.C, rng=np.random.default_rng(3))
    figures = KR.check_real(case.X, case.C, got)                 # the bounds hold for float32 arithmetic of this scheme
    assert 0 < figures["sums"] <= 1 and 0 < figures["inertia"] <= 1
    # ... and not for a node dropped from the LARGEST cluster (where a node weighs least against the bound): the node
    # of median |x|_1 among that cluster's
    lab, counts, sums, outer, inertia = got
    k = int(np.argmax(counts))
    members = np.flatnonzero(lab == k)
    i = members[np.argsort(np.abs(case.X[members]).sum(axis=1))[len(members) // 2]]
    x = case.X[i]
    _, abs_c, _, abs_s, abs_o = KR.moments(case.X, lab, case.K)
    assert np.any(np.abs(x) > KR.sum_bound(abs_s[k], case.n))
    assert np.any(np.abs(np.outer(x, x)) > KR.sum_bound(abs_o[k], case.n))
    d = float(KR.distance_at(case.X[i:i + 1], case.C, lab[i:i + 1])[0])
    dropped = (lab, counts, sums - np.eye(case.K)[k][:, None] * x, outer, inertia)
    with pytest.raises(AssertionError, match="sums"):
        KR.check_real(case.X, case.C, dropped)
    dropped = (lab, counts, sums, outer - np.eye(case.K)[k][:, None, None] * np.outer(x, x), inertia)
    with pytest.raises(AssertionError, match="outer"):
        KR.check_real(case.X, case.C, dropped)
    if d > KR.inertia_bound(case.S, inertia) * 2:
        with pytest.raises(AssertionError, match="inertia"):
            KR.check_real(case.X, case.C, (lab, counts, sums, outer, inertia - d))
    with pytest.raises(AssertionError, match="counts"):
        KR.check_real(case.X, case.C, (lab, counts - np.eye(case.K)[k], sums, outer, inertia))


def test_a_label_without_a_tie_is_refused():
    case = KR.case(*REAL[2])
    lab, counts, sums, outer, inertia = KR.emulate(case.X, case.C)
    _, d1, d2 = KR.two_smallest(case.X, case.C)
    i = int(np.argmax(d2 - d1))
    wrong = lab.copy()
    wrong[i] = (lab[i] + 1) % case.K
    with pytest.raises(AssertionError, match="without a tie"):
        KR.check_real(case.X, case.C, (wrong,) + KR.moments(case.X, wrong, case.K)[:3] + (inertia,))
