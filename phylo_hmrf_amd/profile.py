"""What a state IS: per state and species the exact quantiles, the mean and standard deviation of the observations, the
state's share per chromosome and over the genomic-distance bands -- the numbers behind the per-state box plots
(DESIGN.md section 7).

Everything is taken from what the blocks already hold on the GPU: the f32 observations and the u8 labels.  The order
statistics are EXACT: a radix selection in four passes of 8 bits over the orderable key of the f32 bit pattern
(phmrf_state_hist, include/phmrf.h).  Each pass returns, per (state, species, slot), the histogram of one digit among the
values that match the slot's prefix; `select` below -- pure NumPy, nothing of the GPU in it -- walks every wanted rank one
digit down, lets targets with equal prefixes share a slot and hands the next pass its prefixes.  Counts, sums, sums of squares
and band counts come from one more pass (phmrf_state_moments).

Ordering: that of the key b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000) of the bit pattern b.  -0 sorts below +0 (they are equal
as floats, np.sort may return either in either place) and non-finite values sort to the two ends by their bits, a NaN with
the sign bit set below -inf.  Nothing is inspected or refused.

There is no host fallback: without a GPU `state_profile` raises RuntimeError.
"""
import json
import time

import numpy as np

SENTINEL = 0xFFFFFFFF          # a prefix slot that matches nothing
MAX_SLOTS = 16                 # J of phmrf_state_hist = the most targets per (state, species) of one selection
MAX_QUANTILES = 8              # two order statistics each
BANDS = 32                     # include/phmrf.h PHMRF_DIFF_BANDS
HIST_GRID_CAP = 512            # csrc/profile.hip HIST_GRID_CAP: workgroups of 256 nodes per trip along x
DEFAULT_QUANTILES = (0.003, 0.25, 0.5, 0.75, 0.997)      # the reference's cnt_estimate
SHIFTS = (24, 16, 8, 0)
NPZ_KEYS = ("count", "share", "count_region", "mean", "sd", "quantiles", "q_lo", "q_hi", "q", "bands", "chrom", "enrichment",
            "order", "species", "timing")


def keys_to_float32(keys):
    """the float32 values of orderable keys (uint32): the inverse of b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000)"""
    keys = np.asarray(keys, dtype=np.uint32)
    bits = np.where(keys >> np.uint32(31), keys ^ np.uint32(0x80000000), ~keys)
    return bits.astype(np.uint32).view(np.float32)


def select(run_pass, reduce, count, ranks, dedup=True):
    """The host side of the selection.  run_pass(shift, prefix uint32 [K, S, J]) -> this rank's histogram [K, S, J, 256] summed
    over its units (at shift 24 J is 1 and the prefix means nothing); reduce(array) -> the array summed over the ranks;
    count int64 [K]; ranks int64 [K, S, T], T <= 16, 0-based ranks into the sorted values of (state, species), -1: no such
    rank.  -> float32 [K, S, T], the values np.sort puts at those ranks (NaN where the rank is -1).
    dedup=False gives every target a slot of its own (tests: the result must not change)."""
    ranks = np.asarray(ranks, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    K, S, T = ranks.shape
    if T > MAX_SLOTS:
        raise ValueError("at most %d ranks per (state, species), not %d" % (MAX_SLOTS, T))
    if np.any(ranks >= count[:, None, None]) or np.any(ranks < -1):
        raise ValueError("a rank is outside its state's count")
    valid = ranks >= 0
    residual = np.where(valid, ranks, 0)
    prefix = np.zeros((K, S, T), dtype=np.int64)            # the key's digits found so far
    slot = np.zeros((K, S, T), dtype=np.int64)
    pre = np.zeros((K, S, 1), dtype=np.uint32)
    for shift in SHIFTS:
        if shift != 24:
            # targets of one (k, s) with equal prefixes share a slot; J = the most distinct prefixes of any (k, s)
            table = [[[] for _ in range(S)] for _ in range(K)]
            for k, s, t in zip(*np.nonzero(valid)):
                row = table[k][s]
                p = int(prefix[k, s, t])
                if dedup and p in row:
                    slot[k, s, t] = row.index(p)
                else:
                    slot[k, s, t] = len(row)
                    row.append(p)
            J = max(1, max(len(row) for rows in table for row in rows))
            pre = np.full((K, S, J), SENTINEL, dtype=np.uint32)
            for k in range(K):
                for s in range(S):
                    pre[k, s, :len(table[k][s])] = table[k][s]
        hist = np.asarray(reduce(np.asarray(run_pass(shift, pre)))).reshape(K, S, pre.shape[2], 256)
        cum = np.cumsum(hist.astype(np.int64), axis=3)
        for k, s, t in zip(*np.nonzero(valid)):
            c = cum[k, s, slot[k, s, t]]
            d = int(np.searchsorted(c, residual[k, s, t], side="right"))     # the first digit whose cumulative count passes it
            if d > 255:
                raise RuntimeError("the histograms of state %d, species %d do not hold rank %d: labels or observations "
                                   "changed between the passes" % (k, s, ranks[k, s, t]))
            residual[k, s, t] -= c[d - 1] if d else 0
            prefix[k, s, t] = (prefix[k, s, t] << 8) | d
    out = keys_to_float32(prefix.astype(np.uint32))
    return np.where(valid, out, np.float32(np.nan)).astype(np.float32)


def quantile_ranks(count, quantiles):
    """NumPy's default ("linear") definition: h = (n - 1) q in float64 -> (lo = floor h, hi = ceil h as int64 [K, Q] with -1 for
    an empty state, h - lo as float64 [K, Q])"""
    count = np.asarray(count, dtype=np.int64)
    q = np.asarray(quantiles, dtype=np.float64)
    h = (count[:, None] - 1).astype(np.float64) * q[None, :]
    lo, hi = np.floor(h).astype(np.int64), np.ceil(h).astype(np.int64)
    empty = count[:, None] <= 0
    return np.where(empty, -1, lo), np.where(empty, -1, hi), np.where(empty, 0.0, h - np.floor(h))


def interpolate(q_lo, q_hi, frac):
    """q = q_lo + (h - lo) (q_hi - q_lo) in float64; q_lo itself where the two order statistics are one"""
    a, b = q_lo.astype(np.float64), q_hi.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(frac[:, None, :] == 0.0, a, a + frac[:, None, :] * (b - a))


def moments(count, total, sq):
    """-> (mean, sd with n - 1 in the denominator) float64 [K, S]; NaN for an empty state / fewer than 2 nodes.
    var = (sum x^2 - n mean^2) / (n - 1) in float64: it loses digits as (mean / sd)^2 grows"""
    n = np.asarray(count, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(n > 0, total / n, np.nan)
        var = np.where(n > 1, (sq - n * mean * mean) / (n - 1.0), np.nan)
        sd = np.sqrt(np.maximum(var, 0.0))
    return mean, np.where(n > 1, sd, np.nan)


def enrichment(count_region, chrom_of_region):
    """-> (chrom int64 [C] ascending, enrichment float64 [C, K] = log2(share of state k on chromosome c / genome-wide share
    of k + 1e-16)); NaN for a state that occurs nowhere"""
    count_region = np.asarray(count_region, dtype=np.float64)
    chrom_of_region = np.asarray(chrom_of_region, dtype=np.int64)
    chrom = np.unique(chrom_of_region)
    per = np.stack([count_region[chrom_of_region == c].sum(axis=0) for c in chrom]) if chrom.size else \
        np.zeros((0, count_region.shape[1]))
    with np.errstate(invalid="ignore", divide="ignore"):
        share_c = per / per.sum(axis=1, keepdims=True)
        share = count_region.sum(axis=0) / count_region.sum()
        return chrom, np.log2(share_c / share[None, :] + 1e-16)


def state_order(count, medians):
    """the states by descending mean over the species of the per-species medians [K, S]; empty states last, in ascending
    number (as are states whose medians are not finite)"""
    count = np.asarray(count)
    with np.errstate(invalid="ignore"):
        m = np.mean(np.asarray(medians, dtype=np.float64), axis=1)
    full = [k for k in range(len(count)) if count[k] > 0 and np.isfinite(m[k])]
    rest = [k for k in range(len(count)) if k not in full]
    return np.asarray(sorted(full, key=lambda k: (-m[k], k)) + rest, dtype=np.int64)


def check_quantiles(quantiles):
    q = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    if q.ndim != 1 or not 1 <= q.size <= MAX_QUANTILES or not np.all(np.isfinite(q)) or np.any(q < 0) or np.any(q > 1):
        raise ValueError("quantiles: 1 to %d numbers in [0, 1], not %r" % (MAX_QUANTILES, quantiles))
    return q


def parse_quantiles(text):
    """"0.003,0.25,0.5" -> float64 array (ValueError for anything else)"""
    try:
        q = [float(t) for t in str(text).split(",")]
    except ValueError:
        raise ValueError("quantiles: a comma-separated list of numbers in [0, 1], not %r" % (text,))
    return check_quantiles(q)


def _units(model):
    """(region, Block, dist0 of the block's own cell (0, 0), it is a grid block) of every whole block and row tile this rank
    holds, in a fixed order"""
    out = []
    for r in sorted(model.my_regions):
        lv = model.len_vec[r]
        dist0 = int(lv[6]) - int(lv[5]) if len(lv) > 6 else 0
        out.append((r, model.blocks[r], dist0, r not in model.general_graph_regions, True))
    for g in model.conductor.groups:
        lv = model.len_vec[g.block_id]
        dist0 = int(lv[6]) - int(lv[5]) if len(lv) > 6 else 0
        for t in sorted(g.local):
            tl = g.local[t]
            # rows and columns of a diagonal block's tile shift alike; a full block's tile starts at stored row s0
            out.append((g.block_id, tl.b, dist0 if tl.diag else dist0 - tl.s0, True, False))
    return out


def state_profile(model, quantiles=DEFAULT_QUANTILES, state_vec=None, want_bands=True):
    """The profile of the labelling the device holds (after segment() or a fit), or of `state_vec` (a labelling of all
    samples, uploaded first as the blocks' current labels: a smoothed map, the state_vec a fit wrote).  -> dict:
      count int64 [K], share float64 [K], count_region int64 [R, K]
      mean, sd float64 [K, S] (sd with n - 1; NaN below 2 nodes)
      quantiles float64 [Q]; q_lo, q_hi float32 [K, S, Q] the two exact order statistics at floor / ceil of (n - 1) q;
      q float64 [K, S, Q] = q_lo + (h - lo)(q_hi - q_lo); NaN for an empty state
      bands int64 [K, 32] per band of the genomic distance (grid blocks only; None without want_bands)
      chrom int64 [C], enrichment float64 [C, K]; order int64 [K]; timing {stage: ms}"""
    from . import _lib
    _lib.require_gpu()
    q = check_quantiles(quantiles)
    K, S, R = int(model.n_components), int(model.n_features), len(model.len_vec)
    t_start = time.perf_counter()
    if state_vec is not None:
        sv = np.asarray(state_vec).reshape(-1)
        if sv.shape[0] != int(model.n_samples):
            raise ValueError("state_vec has %d entries, the model %d samples" % (sv.shape[0], int(model.n_samples)))
        model._upload_labels_slot(sv, None)
    units = _units(model)
    whole = [u for u in units if u[4]]
    tiles = [u for u in units if not u[4]]
    red = model.reducer

    def reduce(a):
        a = np.asarray(a)
        return np.rint(red.allreduce(a.astype(np.float64).reshape(-1))).astype(np.int64).reshape(a.shape)

    def over_units(fn):
        """fn(unit) of every unit: whole blocks on the block runner, tiles from this thread; results in the units' order"""
        pending = model.runner.start(fn, whole)
        mine = [fn(u) for u in tiles]
        return pending.results() + mine

    timing = {}
    t0 = time.perf_counter()
    count_region = np.zeros((R, K), dtype=np.int64)
    total, sq = np.zeros((K, S)), np.zeros((K, S))
    bands = np.zeros((K, BANDS), dtype=np.int64) if want_bands else None
    try:
        got = over_units(lambda u: u[1].state_moments(u[2], want_bands and u[3]))
    except _lib.PhmrfError as e:
        if e.status != 5:
            raise
        raise RuntimeError("no labels on the device: run segment() or a fit before state_profile() (%s)" % e)
    for u, (c, s1, s2, bd) in zip(whole + tiles, got):
        count_region[u[0]] += c
        total += s1
        sq += s2
        if bd is not None:
            bands += bd
    if model.world > 1:
        count_region = reduce(count_region)
        total = red.allreduce(total.reshape(-1)).reshape(K, S)
        sq = red.allreduce(sq.reshape(-1)).reshape(K, S)
        if want_bands:
            bands = reduce(bands)
    count = count_region.sum(axis=0)
    timing["moments"] = 1e3 * (time.perf_counter() - t0)

    passes = []

    def run_pass(shift, prefix):
        t1 = time.perf_counter()
        hist = np.zeros((K, S, prefix.shape[2], 256), dtype=np.int64)
        for h in over_units(lambda u: u[1].state_hist(shift, prefix)):
            hist += h.astype(np.int64)
        passes.append(dict(shift=shift, J=int(prefix.shape[2]), ms=1e3 * (time.perf_counter() - t1)))
        return hist

    lo, hi, frac = quantile_ranks(count, q)
    Q = q.size
    ranks = np.broadcast_to(np.concatenate([lo, hi], axis=1)[:, None, :], (K, S, 2 * Q))
    stat = select(run_pass, reduce, count, ranks)
    q_lo, q_hi = stat[:, :, :Q], stat[:, :, Q:]
    qv = interpolate(q_lo, q_hi, frac)
    at_half = np.nonzero(q == 0.5)[0]
    if at_half.size:
        med = qv[:, :, at_half[0]]
    else:
        mlo, mhi, mfrac = quantile_ranks(count, [0.5])
        ms = select(run_pass, reduce, count, np.broadcast_to(np.concatenate([mlo, mhi], axis=1)[:, None, :], (K, S, 2)))
        med = interpolate(ms[:, :, :1], ms[:, :, 1:], mfrac)[:, :, 0]
    timing["passes"] = passes
    mean, sd = moments(count, total, sq)
    chrom_of_region = [int(lv[9]) if len(lv) > 9 else 0 for lv in model.len_vec]
    chrom, enr = enrichment(count_region, chrom_of_region)
    n_all = max(int(count.sum()), 1)
    timing["total"] = 1e3 * (time.perf_counter() - t_start)
    return dict(count=count, share=count / float(n_all), count_region=count_region, mean=mean, sd=sd, quantiles=q, q_lo=q_lo,
                q_hi=q_hi, q=qv, bands=bands, chrom=chrom, enrichment=enr, order=state_order(count, med), timing=timing)


def save_npz(path, prof, species=None):
    """the result of state_profile() as an .npz without pickles: NPZ_KEYS (bands empty [0, 32] when not computed, species the
    leaf names or empty, timing as a JSON string)"""
    bands = prof["bands"] if prof.get("bands") is not None else np.zeros((0, BANDS), dtype=np.int64)
    np.savez(path, count=np.asarray(prof["count"], dtype=np.int64), share=np.asarray(prof["share"], dtype=np.float64),
             count_region=np.asarray(prof["count_region"], dtype=np.int64), mean=np.asarray(prof["mean"], dtype=np.float64),
             sd=np.asarray(prof["sd"], dtype=np.float64), quantiles=np.asarray(prof["quantiles"], dtype=np.float64),
             q_lo=np.asarray(prof["q_lo"], dtype=np.float32), q_hi=np.asarray(prof["q_hi"], dtype=np.float32),
             q=np.asarray(prof["q"], dtype=np.float64), bands=np.asarray(bands, dtype=np.int64),
             chrom=np.asarray(prof["chrom"], dtype=np.int64), enrichment=np.asarray(prof["enrichment"], dtype=np.float64),
             order=np.asarray(prof["order"], dtype=np.int64),
             species=np.asarray([] if species is None else [str(s) for s in species], dtype=np.str_),
             timing=np.asarray(json.dumps(prof.get("timing", {}))))
    return path


def load_npz(path):
    """-> dict with NPZ_KEYS; species a list of str, timing a dict, bands None when they were not computed"""
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k].copy() for k in NPZ_KEYS}
    d["species"] = [str(s) for s in d["species"].tolist()]
    d["timing"] = json.loads(str(d["timing"]))
    if d["bands"].shape[0] == 0 and d["count"].shape[0] != 0:
        d["bands"] = None
    return d


def text_lines(prof, species=None):
    """one tab-separated line per state and species: state + 1, species, count, share, mean, sd, the quantiles, the state's
    position in `order` (0: the highest median); a header line first"""
    K, S = prof["mean"].shape
    names = [str(s) for s in species] if species is not None and len(species) == S else ["species%d" % (s + 1) for s in range(S)]
    pos = np.empty(K, dtype=np.int64)
    pos[np.asarray(prof["order"])] = np.arange(K)
    lines = ["#state\tspecies\tcount\tshare\tmean\tsd\t%s\torder\n" % "\t".join("q%g" % v for v in prof["quantiles"])]
    for k in range(K):
        for s in range(S):
            qs = "\t".join("%.9g" % v for v in prof["q"][k, s])
            lines.append("%d\t%s\t%d\t%.6g\t%.9g\t%.9g\t%s\t%d\n" % (k + 1, names[s], prof["count"][k], prof["share"][k],
                                                                 prof["mean"][k, s], prof["sd"][k, s], qs, pos[k]))
    return lines


def save_txt(path, prof, species=None):
    with open(path, "w") as f:
        f.writelines(text_lines(prof, species))
    return path
