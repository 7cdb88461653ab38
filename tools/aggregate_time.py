#!/usr/bin/env python3
"""Time the rescaled pile-up of a state map (phmrf_state_aggregate) on tools/enrich_time.py's genome map (default cfg3: whole
genome at 50 kb, 26 blocks, 88.8 M nodes, K = 20) at a body of --body (32) and a flank of --flank (16) cells with three lists:

    tads     consecutive intervals of 10 .. 40 bins that tile every chromosome (about 3,000): one group
    domains  consecutive intervals of 100 .. 500 bins that tile every chromosome (about 200) with their controls --shift (100)
             bins along the diagonal to either side (with_controls): two groups
    large    consecutive intervals of 600 .. 2,000 bins that tile every chromosome (about 100): one group.  At a body of 32
             ceil(600 / 32)^2 = 361 > SMALL_AREA, so every one of them goes a wave per pile cell (aggregate_wave_kernel); the
             other two lists stay with the lane kernel

The map and every chromosome's features are on the GPU before anything is timed.  Per list, summed over the chromosomes, in
milliseconds by HIP events around the library call (each call allocates and zeroes its tables, uploads its regions, runs its
two kernels and copies both tables to the host before it returns), the fastest of --repeats.  Beside it, on --subset features
of the list taken at even steps and scaled by features / subset:
    rect_ms  `cells` alone through phmrf_rect_states: one rectangle per (feature, pile cell, orientation, region) and one
             single-bin rectangle subtracted per bin pair (p, p) of a mirrored cell, one output row per (feature, pile cell);
             the rectangle lists are made before the clock starts
    host_ms  the NumPy restatement of tests/aggregate_reference.py on this machine's CPU
The three tables of the subset (the device's from a call of its own) must be equal: cells of all three, votes of the device
and the host.  One JSON object, printed and written to --out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
NOT_MEASURED = ["the kernels' own time apart from the call's fixed cost (no kernel trace was taken): allocation, the memset, the "
                "copies of the two tables and the waits are inside every figure",
                "the threshold between the lane-per-cell and the wave-per-cell kernel (SMALL_AREA = 256 is the largest the 16-bit "
                "counters allow; no other value was run)",
                "the chunk length (CHUNK = 256) and the tile (LANES = 128), the grid caps",
                "other K than the workload's 20, other grids than --body / --flank",
                "state_aggregate / aggregate_files end to end (host -> device, the readers, the sum over chromosomes, the text, the images)",
                "bytes moved and the share of the HBM peak", "the spread between runs (the fastest of --repeats counts)"]


def tiling(bins, lo, hi, rng):
    """-> int64 [N, 7]: consecutive intervals of lo .. hi bins that tile every chromosome, group 0, not flipped"""
    rows = []
    for c in sorted(bins):
        at = 0
        while at + lo <= bins[c]:
            n = min(int(rng.integers(lo, hi + 1)), bins[c] - at)
            rows.append([c, at, at + n, at, at + n, 0, 0])
            at += n
    return np.array(rows, dtype=np.int64)


def rect_lists(lv, features, T, F):
    """-> per region that some feature touches (the len_vec row, rect, slot, minus): phmrf_rect_states' arguments for the `cells`
    of the features, the output row of (feature t, pile cell (u, v)) being t P P + u P + v"""
    from phylo_hmrf_amd import aggregate
    P = T + 2 * F
    lists = []
    for row in lv:
        s1, s2 = int(row[5]), int(row[6])
        rect, slot, minus = [], [], []
        for t, f in enumerate(features):
            if f[0] != row[9]:
                continue
            alo, ahi = aggregate.axis_cells(f[1], f[2], T, F)
            blo, bhi = aggregate.axis_cells(f[3], f[4], T, F)
            for u in range(P):
                for v in range(P):
                    uu, vv = (P - 1 - u, P - 1 - v) if f[6] else (u, v)
                    at = t * P * P + u * P + v
                    rect += [[alo[uu] - s1, ahi[uu] - s1, blo[vv] - s2, bhi[vv] - s2], [blo[vv] - s1, bhi[vv] - s1, alo[uu] - s2, ahi[uu] - s2]]
                    slot += [at, at]
                    minus += [0, 0]
                    for p in range(max(alo[uu], blo[vv]), min(ahi[uu], bhi[vv])):      # (p, p) does not count a second time
                        rect.append([p - s1, p - s1 + 1, p - s2, p - s2 + 1])
                        slot.append(at)
                        minus.append(1)
        if not rect:
            continue
        lists.append((row, np.clip(np.array(rect, dtype=np.int64), -(1 << 29), 1 << 29), np.array(slot, dtype=np.int64),
                      np.array(minus, dtype=np.uint8)))
    return lists


def rect_cells(lib, stream, m_t, K, lists, n_features, P):
    """`cells` of the features (one group) through phmrf_rect_states, one call per region of rect_lists -> int64 [P, P, K]"""
    from phylo_hmrf_amd import query
    per_feature = np.zeros((n_features * P * P, K), dtype=np.int64)
    for row, rect, slot, minus in lists:
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        rows, counts, _ = query.region_states(lib, stream, ctypes.c_void_p(m_t[lo:hi].data_ptr()), None, H, W, diag, K, rect, slot, minus)
        per_feature[rows] += counts
    return per_feature.reshape(n_features, P, P, K).sum(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--body", type=int, default=32)
    ap.add_argument("--flank", type=int, default=16)
    ap.add_argument("--shift", type=int, default=100, help="domains: the controls' shift in bins")
    ap.add_argument("--subset", type=int, default=6, help="features of every list the two baselines take")
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of every call; the fastest counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_time.json"))
    a = ap.parse_args()
    import torch
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib, aggregate
    from tests import aggregate_reference
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    T, F = a.body, a.flank
    P = T + 2 * F

    def prepare(lv, features, G):
        """-> per chromosome with features: (regions, offsets, the features and the flips on the device, how many)"""
        calls = []
        for c in np.unique(lv[:, 9]):
            sel = features[features[:, 0] == c]
            if not sel.shape[0]:
                continue
            sel = sel[np.argsort(sel[:, 5], kind="stable")]
            offsets = np.concatenate([[0], np.cumsum(np.bincount(sel[:, 5], minlength=G))]).astype(np.int64)
            regs = np.ascontiguousarray(lv[lv[:, 9] == c][:, [1, 3, 4, 5, 6, 8]], dtype=np.int64)
            calls.append((regs, offsets, torch.from_numpy(np.ascontiguousarray(sel[:, 1:5], dtype=np.int32)).to(dev),
                          torch.from_numpy(np.ascontiguousarray(sel[:, 6], dtype=np.uint8)).to(dev), sel.shape[0]))
        return calls

    def call(m_t, n, K, G, one):
        regs, offsets, feat_t, flip_t, _ = one
        cells, votes = np.zeros((G, P, P, K), dtype=np.int64), np.zeros((G, P, P, K), dtype=np.int64)
        _lib.check(L.phmrf_state_aggregate(ctypes.c_void_p(m_t.data_ptr()), n, regs.shape[0], _lib.ptr_i64(regs), K, T, F, G,
                                           _lib.ptr_i64(offsets), ctypes.c_void_p(feat_t.data_ptr()), ctypes.c_void_p(flip_t.data_ptr()),
                                           _lib.ptr_i64(cells), _lib.ptr_i64(votes), st))
        return cells, votes

    def timed(fn):
        best = None
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        return best, out

    def run(name, m_t, sv, lv, K, features, G):
        ms, cells, votes = 0.0, 0, 0
        calls = prepare(lv, features, G)
        for one in calls:
            t, (c, v) = timed(lambda: call(m_t, sv.size, K, G, one))
            ms += t
            cells, votes = cells + c, votes + v
        na, nb = features[:, 2] - features[:, 1], features[:, 4] - features[:, 3]
        small = int(sum(aggregate.is_small(x, y, T) for x, y in zip(na, nb)))
        # the baselines: a subset of the first group, at even steps
        first = features[features[:, 5] == 0]
        sub = first[np.linspace(0, first.shape[0] - 1, min(a.subset, first.shape[0])).astype(np.int64)]
        got_c, got_v = 0, 0
        for one in prepare(lv, sub, 1):
            c, v = call(m_t, sv.size, K, 1, one)
            got_c, got_v = got_c + c, got_v + v
        t0 = time.perf_counter()
        host_c, host_v = aggregate_reference.state_aggregate(sv, lv, sub, T, F, K, 1)
        host_ms = 1e3 * (time.perf_counter() - t0)
        lists = rect_lists(lv, sub, T, F)
        rect_ms, rect_c = timed(lambda: rect_cells(L, st, m_t, K, lists, sub.shape[0], P))
        agree = bool(np.array_equal(got_c, host_c) and np.array_equal(got_v, host_v) and np.array_equal(got_c[0], rect_c))
        scale = features.shape[0] / sub.shape[0]
        res = dict(features=int(features.shape[0]), groups=G, body=T, flank=F, pile_cells=P * P, calls=len(calls), small_features=small,
                   wave_features=int(features.shape[0]) - small, bins=[int(na.min()), int(na.max())], bin_pairs=int(np.sum(cells)),
                   votes=int(np.sum(votes)), ms=round(ms, 3), subset=int(sub.shape[0]), subset_rect_ms=round(rect_ms, 1),
                   subset_host_ms=round(host_ms, 1), rect_ms_scaled=round(rect_ms * scale, 1), host_ms_scaled=round(host_ms * scale, 1),
                   tables_agree=agree, rect_over_device=round(rect_ms * scale / ms, 1), host_over_device=round(host_ms * scale / ms, 1))
        print("%s: %s" % (name, json.dumps(res)), flush=True)
        assert agree, "%s: the three tables of the subset differ" % name
        return res

    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    print("genome maps ready: %d nodes" % sv.size, flush=True)
    m_t = torch.from_numpy(sv).to(dev)
    chroms = [int(c) for c in np.unique(lv[:, 9])]
    bins = {c: max(max(int(r[5] + r[3]), int(r[6] + r[4])) for r in lv if r[9] == c) for c in chroms}
    rng = np.random.default_rng(a.seed + 11)
    tads = tiling(bins, 10, 40, rng)
    domains = aggregate.with_controls(tiling(bins, 100, 500, rng), a.shift, 1)
    call(m_t, sv.size, K, 1, prepare(lv, tads[:4], 1)[0])        # (code objects loaded before the first timing)
    out = dict(repeats=a.repeats, host_threads=min(16, os.cpu_count() or 1), workload=a.workload, desc=desc, noise=a.noise,
               nodes=int(sv.size), blocks=int(lv.shape[0]), K=K, inputs={})
    out["inputs"]["tads"] = run("tads", m_t, sv, lv, K, tads, 1)
    out["inputs"]["domains"] = dict(run("domains", m_t, sv, lv, K, domains, 2), shift=a.shift)
    large = tiling(bins, 600, 2000, rng)
    out["inputs"]["large"] = run("large", m_t, sv, lv, K, large, 1)
    out["not_measured"] = NOT_MEASURED
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
