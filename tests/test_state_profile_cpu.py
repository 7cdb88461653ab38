"""CPU: the host side of the state profile (phylo_hmrf_amd/profile.py) -- the four-pass radix selection driven by the NumPy
restatement of phmrf_state_hist, slot deduplication, two emulated ranks, the interpolated quantiles against np.quantile,
enrichment / order / .npz / .txt on a hand-worked case, and the command line's refusals."""
import os

import numpy as np
import pytest

from phylo_hmrf_amd import profile as P
from tests import state_profile_reference as SR


def _group(seed, form, sizes, S=2):
    """observations and labels with state k holding sizes[k] nodes (0: an empty state), shuffled"""
    rng = np.random.default_rng(seed)
    labels = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(labels)
    x32 = SR.make_values(form, rng, labels.size, S).astype(np.float32)
    return x32, labels, np.asarray(sizes, dtype=np.int64)


def _all_ranks(count, S, T, rng):
    """T ranks per (k, s): the ends, and random ones; -1 for an empty state"""
    K = count.size
    ranks = np.full((K, S, T), -1, dtype=np.int64)
    for k in range(K):
        if count[k] > 0:
            r = rng.integers(0, count[k], (S, T))
            r[:, 0], r[:, -1] = 0, count[k] - 1
            ranks[k] = r
    return ranks


CASES = [(form, sizes) for form in SR.FORMS for sizes in ([700, 0, 1, 37], [1], [257], [64, 65, 3, 2, 129])]


@pytest.mark.parametrize("form,sizes", CASES)
def test_select_returns_the_sorted_values(form, sizes):
    x32, labels, count = _group(len(form) + sum(sizes), form, sizes)
    K, S = count.size, x32.shape[1]
    ranks = _all_ranks(count, S, 6, np.random.default_rng(1))
    run_pass, log = SR.make_run_pass([(x32, labels)], K)
    got = P.select(run_pass, lambda a: a, count, ranks)
    assert got.dtype == np.float32 and got.shape == ranks.shape
    assert [s for s, _ in log] == [24, 16, 8, 0]
    for k in range(K):
        for s in range(S):
            v = np.sort(x32[labels == k, s])
            for t in range(ranks.shape[2]):
                if ranks[k, s, t] < 0:
                    assert np.isnan(got[k, s, t])
                else:
                    assert got[k, s, t] == v[ranks[k, s, t]]
    # bit for bit the key order's value (-0 below +0, which np.sort does not tell apart)
    want = SR.order_statistics(x32, labels, K, ranks)
    assert np.array_equal(got.view(np.uint32)[ranks >= 0], want.view(np.uint32)[ranks >= 0])


def test_select_every_rank_of_small_groups():
    """every rank of groups of 1 .. 16 values, all forms"""
    for form in SR.FORMS:
        for n in range(1, 17):
            x32, labels, count = _group(n, form, [n], S=1)
            ranks = np.full((1, 1, 16), -1, dtype=np.int64)
            ranks[0, 0, :n] = np.arange(n)
            run_pass, _ = SR.make_run_pass([(x32, labels)], 1)
            got = P.select(run_pass, lambda a: a, count, ranks)
            assert np.array_equal(got[0, 0, :n].view(np.uint32), SR.key_sort(x32[:, 0]).view(np.uint32)), (form, n)


@pytest.mark.parametrize("form", SR.FORMS)
def test_slots_are_shared_by_equal_prefixes(form):
    x32, labels, count = _group(5, form, [300, 0, 2])
    K, S = 3, 2
    ranks = _all_ranks(count, S, 16, np.random.default_rng(2))
    run_pass, log = SR.make_run_pass([(x32, labels)], K)
    got = P.select(run_pass, lambda a: a, count, ranks)
    keys = SR.order_key(SR.order_statistics(x32, labels, K, ranks)).astype(np.int64)
    for shift, prefix in log[1:]:
        distinct = max(len(set((keys[k, s, ranks[k, s] >= 0] >> (shift + 8)).tolist())) for k in range(K) for s in range(S))
        assert prefix.shape[2] == max(distinct, 1)                 # never more slots than distinct prefixes
        for k in range(K):
            for s in range(S):
                row = [p for p in prefix[k, s].tolist() if p != P.SENTINEL]
                assert len(row) == len(set(row))
                assert all(p == P.SENTINEL for p in prefix[k, s, len(row):].tolist())
    run_plain, log_plain = SR.make_run_pass([(x32, labels)], K)
    plain = P.select(run_plain, lambda a: a, count, ranks, dedup=False)
    assert all(prefix.shape[2] == 16 for _, prefix in log_plain[1:])
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


def test_two_emulated_ranks_equal_one():
    x32, labels, count = _group(9, "normal", [400, 90, 0, 1])
    K, S = 4, 2
    ranks = _all_ranks(count, S, 10, np.random.default_rng(3))
    one, _ = SR.make_run_pass([(x32, labels)], K)
    single = P.select(one, lambda a: a, count, ranks)
    half = labels.size // 2
    first, _ = SR.make_run_pass([(x32[:half], labels[:half])], K)
    second, _ = SR.make_run_pass([(x32[half:], labels[half:])], K)
    state = {}

    def run_pass(shift, prefix):                   # rank 0's histogram; rank 1's waits for the reduction
        state["other"] = second(shift, prefix)
        return first(shift, prefix)

    def reduce(a):                                 # the model's Reducer sums float64
        return (np.asarray(a, dtype=np.float64) + np.asarray(state["other"], dtype=np.float64)).astype(np.int64)

    both = P.select(run_pass, reduce, count, ranks)
    assert np.array_equal(single.view(np.uint32), both.view(np.uint32))


def test_select_refuses_what_it_cannot_do():
    with pytest.raises(ValueError):
        P.select(None, None, np.array([5]), np.zeros((1, 1, 17), dtype=np.int64))
    with pytest.raises(ValueError):
        P.select(None, None, np.array([5]), np.full((1, 1, 2), 5, dtype=np.int64))


@pytest.mark.parametrize("form", SR.FORMS)
def test_interpolated_quantiles_against_numpy(form):
    """q against np.quantile on the float64 of the values: two float64 roundings on either side, 4 * 2^-52 * max(|q_lo|,
    |q_hi|) bounds their difference (a NumPy model of the scheme measured 0.89 * 2^-52 at worst)"""
    quantiles = np.array([0.0, 0.003, 0.25, 0.5, 0.6180339887, 0.75, 0.997, 1.0])
    x32, labels, count = _group(11, form, [700, 0, 1, 2, 333])
    K, S = count.size, x32.shape[1]
    lo, hi, frac = P.quantile_ranks(count, quantiles)
    ranks = np.broadcast_to(np.concatenate([lo, hi], axis=1)[:, None, :], (K, S, 16))
    run_pass, _ = SR.make_run_pass([(x32, labels)], K)
    stat = P.select(run_pass, lambda a: a, count, ranks)
    q_lo, q_hi = stat[:, :, :8], stat[:, :, 8:]
    q = P.interpolate(q_lo, q_hi, frac)
    worst = 0.0
    for k in range(K):
        for s in range(S):
            if count[k] == 0:
                assert np.all(np.isnan(q[k, s]))
                continue
            ref = np.quantile(x32[labels == k, s].astype(np.float64), quantiles)
            scale = np.maximum(np.abs(q_lo[k, s]), np.abs(q_hi[k, s])).astype(np.float64)
            err = np.abs(q[k, s] - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.nanmax(np.where(scale > 0, err / scale, 0.0))))
            assert np.all(err <= 4 * 2.0 ** -52 * scale), (k, s, err, scale)
    print("worst |q - np.quantile| / max(|q_lo|, |q_hi|) = %.3g * 2^-52" % (worst * 2.0 ** 52))


def _hand_profile():
    """K = 3 (state 2 empty), S = 2, two chromosomes"""
    count_region = np.array([[6, 2, 0], [2, 6, 0], [4, 4, 0]], dtype=np.int64)       # regions on chromosomes 1, 1, 2
    chrom, enr = P.enrichment(count_region, [1, 1, 2])
    count = count_region.sum(axis=0)
    q = np.zeros((3, 2, 3))
    q[0, :, 1] = [1.0, 3.0]                  # medians: state 0 -> mean 2, state 1 -> mean 2.5
    q[1, :, 1] = [2.0, 3.0]
    q[2] = np.nan
    mean, sd = P.moments(count, np.array([[12.0, 36.0], [24.0, 36.0], [0.0, 0.0]]),
                         np.array([[12.0 + 11, 108.0 + 44], [48.0, 108.0], [0.0, 0.0]]))
    return dict(count=count, share=count / 24.0, count_region=count_region, mean=mean, sd=sd,
                quantiles=np.array([0.25, 0.5, 0.75]), q_lo=q.astype(np.float32), q_hi=q.astype(np.float32), q=q, bands=None,
                chrom=chrom, enrichment=enr, order=P.state_order(count, q[:, :, 1]), timing=dict(total=1.5))


def test_enrichment_order_and_moments_by_hand():
    p = _hand_profile()
    assert p["chrom"].tolist() == [1, 2]
    # chromosome 1 holds 8 of state 0 among 16 nodes, the genome 12 among 24: fold 1; chromosome 2: 4 of 8, fold 1
    assert np.allclose(p["enrichment"][:, 0], np.log2(np.array([1.0, 1.0]) + 1e-16), rtol=0, atol=1e-15)
    count_region = np.array([[9, 1], [1, 5]])
    chrom, enr = P.enrichment(count_region, [7, 3])
    assert chrom.tolist() == [3, 7]
    # genome shares 10/16 and 6/16; chromosome 3 (the second region): 1/6 and 5/6; chromosome 7: 9/10 and 1/10
    want = np.log2(np.array([[(1 / 6) / (10 / 16), (5 / 6) / (6 / 16)], [0.9 / (10 / 16), 0.1 / (6 / 16)]]) + 1e-16)
    assert np.allclose(enr, want, rtol=0, atol=1e-14)
    assert p["order"].tolist() == [1, 0, 2]            # by descending mean of the medians; the empty state last
    assert P.state_order(np.array([0, 3, 0, 3]), np.array([[np.nan], [1.0], [np.nan], [1.0]])).tolist() == [1, 3, 0, 2]
    assert p["mean"][0].tolist() == [1.0, 3.0] and np.all(np.isnan(p["mean"][2]))
    assert np.allclose(p["sd"][0], [1.0, 2.0]) and p["sd"][1].tolist() == [0.0, 0.0]      # var = 11 / 11, 44 / 11
    assert np.all(np.isnan(P.moments(np.array([1]), np.array([[2.0]]), np.array([[4.0]]))[1]))


def test_npz_round_trip_and_text_lines(tmp_path):
    p = _hand_profile()
    path = P.save_npz(str(tmp_path / "profile.npz"), p, ["human", "chimp"])
    back = P.load_npz(path)
    assert sorted(back) == sorted(P.NPZ_KEYS)
    assert back["species"] == ["human", "chimp"] and back["bands"] is None and back["timing"] == dict(total=1.5)
    for k in ("count", "share", "count_region", "mean", "sd", "quantiles", "q_lo", "q_hi", "q", "chrom", "enrichment", "order"):
        assert np.array_equal(back[k], p[k], equal_nan=True) and back[k].dtype == np.asarray(p[k]).dtype, k
    p["bands"] = np.arange(96).reshape(3, 32)
    assert np.array_equal(P.load_npz(P.save_npz(path, p))["bands"], p["bands"])
    lines = P.text_lines(p, ["human", "chimp"])
    assert lines[0] == "#state\tspecies\tcount\tshare\tmean\tsd\tq0.25\tq0.5\tq0.75\torder\n"
    assert len(lines) == 1 + 3 * 2
    assert lines[1] == "1\thuman\t12\t0.5\t1\t1\t0\t1\t0\t1\n"           # state 1 is second in `order`
    assert lines[4] == "2\tchimp\t12\t0.5\t3\t0\t0\t3\t0\t0\n"
    assert lines[5].split("\t")[:3] == ["3", "human", "0"] and lines[5].split("\t")[4] == "nan"
    out = P.save_txt(str(tmp_path / "profile.txt"), p)
    assert open(out).read().splitlines()[1].split("\t")[1] == "species1"


def test_quantile_lists():
    assert P.parse_quantiles("0.003,0.25,0.5,0.75,0.997").tolist() == list(P.DEFAULT_QUANTILES)
    for bad in ("", "a,b", "0.5,1.5", "-0.1", "nan", ",".join(["0.5"] * 9)):
        with pytest.raises(ValueError):
            P.parse_quantiles(bad)


def test_state_profile_needs_a_gpu(monkeypatch):
    from phylo_hmrf_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(RuntimeError) as e:
        P.state_profile(object())
    assert "no CPU fallback" in str(e.value)


def _cli(**extra):
    import phylo_hmrf as cli
    return cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", "unused", quiet="1", **extra)


@pytest.mark.parametrize("extra,word", [
    (dict(profile="1", postprocess="a.mat"), "--postprocess"),
    (dict(profile="1", compare="a.mat", compare_with="b.mat"), "--compare"),
    (dict(profile="1", profile_quantiles="0.5,x"), "--profile_quantiles"),
    (dict(profile="1", profile_quantiles="0.5,1.01"), "--profile_quantiles"),
    (dict(profile="1", profile_quantiles=",".join(["0.1"] * 9)), "--profile_quantiles"),
    (dict(profile="2"), "--profile"),
])
def test_cli_refusals(extra, word):
    with pytest.raises(SystemExit) as e:
        _cli(**extra)
    assert word in str(e.value)
    assert not os.path.exists("unused")


def test_cli_parses_the_options_with_their_defaults():
    import phylo_hmrf as cli
    o = cli.parse_args([])
    assert (o.profile, o.profile_quantiles) == ("0", "0.003,0.25,0.5,0.75,0.997")
    o = cli.parse_args(["--profile", "1", "--profile_quantiles", "0.1,0.9"])
    assert (o.profile, o.profile_quantiles) == ("1", "0.1,0.9")
