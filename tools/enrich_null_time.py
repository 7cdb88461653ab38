#!/usr/bin/env python3
"""Time the enrichment's permutation null (phmrf_pair_enrichment_null) on tools/enrich_time.py's genome map and annotation
(default cfg3: whole genome at 50 kb, 26 blocks, 88.8 M nodes, K = 20; three classes in intervals of 100 .. 500 bins, every
interval a segment of its own), with --shifts T = 1000 circular shifts per chromosome (at least --min-shift bins), for the
unlimited window and for the window 0 .. --window bins (40: 2 Mb at 50 kb).

The map, the chromosomes' annotation and the weights are on the GPU or ready before anything is timed.  Three times per
window, in milliseconds:

    null     HIP events around the calls of all regions (one call per region: T <= 4096), the fastest of --repeats
    loop     what the library offered before: per shift one phmrf_pair_enrichment call per region over the rolled annotation
             (uploaded per shift, the map resident), HIP events around --base-shifts shifts, scaled to T
    host     np.bincount over the index arrays of the stored nodes inside the window (tools/enrich_time.py's host_tables) per
             shift and region, the host's clock around --host-shifts shifts, scaled to T

and the ratios loop / null and host / null.  The loop's tables of its shifts must equal the null's (obs; expq against the
exact integer product of the loop's cat_dist with the weights).  One JSON object, printed and written to --out.
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
NOT_MEASURED = ["the two kernels' own time apart from the call (no kernel trace was taken): allocation, the memset, the weights' "
                "upload, the copies back and the waits are inside `null`", "the vector pipe's share against the LDS's in the counting "
                "kernel", "other K and C than the workload's 20 and 3 (the shifts of a group, 16 here, fall to 1 at K = 64, C = 8)",
                "other windows than the two, other T", "enrichment_null / enrich_files end to end (the first pass, the upload of the "
                "map, the statistics, the text)", "random maps and per-bin annotations (the runs of equal bins are shortest there)",
                "the spread between runs (the fastest of --repeats counts)"]
C = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--shifts", type=int, default=1000)
    ap.add_argument("--min-shift", type=int, default=20, help="the smallest shift in bins (1 Mb at 50 kb)")
    ap.add_argument("--window", type=int, default=40, help="the second window: 0 .. this many bins")
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of the null; the fastest counts")
    ap.add_argument("--base-shifts", type=int, default=20, help="shifts the loop over phmrf_pair_enrichment is timed on")
    ap.add_argument("--host-shifts", type=int, default=5, help="shifts the host's restatement is timed on (0: leave it out)")
    ap.add_argument("--chunk", type=int, default=256, help="storage rows the host's restatement takes at a time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enrich_null_time.json"))
    a = ap.parse_args()
    import torch
    from enrich_time import annotation, host_tables
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib, enrich
    from phylo_hmrf_amd.tracks import covered_bins
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P, T = 2 * C * C, a.shifts
    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    print("genome maps ready: %d nodes" % sv.size, flush=True)
    m_t = torch.from_numpy(sv).to(dev)
    chroms = sorted(int(c) for c in np.unique(lv[:, 9]))
    bins = {c: int(covered_bins(lv, c).shape[0]) for c in chroms}
    ann = {c: annotation(bins[c], a.seed + 100 + c) for c in chroms}
    ann_t = {c: tuple(torch.from_numpy(x).to(dev) for x in ann[c]) for c in chroms}
    shifts = enrich.draw_shifts(lv, T, min_shift=a.min_shift, seed=a.seed)
    shifts32 = {c: np.ascontiguousarray(v, dtype=np.int32) for c, v in shifts.items()}

    def region(row):
        return tuple(int(row[k]) for k in (1, 2, 3, 4, 5, 6, 8, 9))

    def pass_once(cls_t, seg_t, d_min, d_max, ranges, d0, Dg):
        """one phmrf_pair_enrichment call per region -> (obs [P, K], state_dist [Dg, K], cat_dist [Dg, P])"""
        obs, sd, cd = np.zeros((P, K), dtype=np.int64), np.zeros((Dg, K), dtype=np.int64), np.zeros((Dg, P), dtype=np.int64)
        for row, rng in zip(lv, ranges):
            if rng is None:
                continue
            lo, hi, H, W, s1, s2, diag, chrom = region(row)
            o, s_, c_ = np.zeros((P, K), dtype=np.int64), np.zeros((rng[1], K), dtype=np.int64), np.zeros((rng[1], P), dtype=np.int64)
            _lib.check(L.phmrf_pair_enrichment(
                ctypes.c_void_p(m_t[lo:hi].data_ptr()), H, W, diag, s2 - s1, K, C, ctypes.c_void_p(cls_t[chrom][s1:].data_ptr()),
                ctypes.c_void_p(cls_t[chrom][s2:].data_ptr()), ctypes.c_void_p(seg_t[chrom][s1:].data_ptr()),
                ctypes.c_void_p(seg_t[chrom][s2:].data_ptr()), d_min, d_max, rng[0], rng[1], _lib.ptr_i64(o), _lib.ptr_i64(s_),
                _lib.ptr_i64(c_), st))
            obs += o
            sd[rng[0] - d0:rng[0] - d0 + rng[1]] += s_
            cd[rng[0] - d0:rng[0] - d0 + rng[1]] += c_
        return obs, sd, cd

    def null_once(w, d_min, d_max, ranges, d0, count):
        """one phmrf_pair_enrichment_null call per region with the first `count` shifts -> (null_obs, null_expq) [count, P, K]"""
        null_obs, null_expq = np.zeros((count, P, K), dtype=np.int64), np.zeros((count, P, K), dtype=np.int64)
        for row, rng in zip(lv, ranges):
            if rng is None:
                continue
            lo, hi, H, W, s1, s2, diag, chrom = region(row)
            w_r = np.ascontiguousarray(w[rng[0] - d0:rng[0] - d0 + rng[1]])
            o, e = np.zeros((count, P, K), dtype=np.int64), np.zeros((count, P, K), dtype=np.int64)
            _lib.check(L.phmrf_pair_enrichment_null(
                ctypes.c_void_p(m_t[lo:hi].data_ptr()), H, W, diag, s1, s2, K, C, ctypes.c_void_p(ann_t[chrom][0].data_ptr()),
                ctypes.c_void_p(ann_t[chrom][1].data_ptr()), bins[chrom], _lib.ptr_i32(shifts32[chrom][:count]), count, d_min, d_max,
                rng[0], rng[1], w_r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _lib.ptr_i64(o), _lib.ptr_i64(e), st))
            null_obs += o
            null_expq += e
        return null_obs, null_expq

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def run(label, d_min, d_max):
        ranges = [enrich.distance_range(r[3], r[4], int(r[8]), int(r[6]) - int(r[5]), d_min, d_max) for r in lv]
        held = [g for g in ranges if g is not None]
        d0 = min(g[0] for g in held)
        Dg = max(g[0] + g[1] for g in held) - d0
        cls0, seg0 = {c: ann_t[c][0] for c in chroms}, {c: ann_t[c][1] for c in chroms}
        obs, sd, cd = pass_once(cls0, seg0, d_min, d_max, ranges, d0, Dg)
        w = enrich.weights(sd)
        null_once(w, d_min, d_max, ranges, d0, 1)            # (code objects loaded before the first timing)
        null_ms, got = None, None
        for _ in range(a.repeats):
            ms, got = events(lambda: null_once(w, d_min, d_max, ranges, d0, T))
            null_ms = ms if null_ms is None else min(null_ms, ms)
        null_obs, null_expq = got
        nodes = int(obs.sum())

        def loop():                                          # the first --base-shifts shifts by the entry point of before
            out = []
            for t in range(a.base_shifts):
                cls_t = {c: torch.from_numpy(np.roll(ann[c][0], -int(shifts[c][t]))).to(dev) for c in chroms}
                seg_t = {c: torch.from_numpy(np.roll(ann[c][1], -int(shifts[c][t]))).to(dev) for c in chroms}
                out.append(pass_once(cls_t, seg_t, d_min, d_max, ranges, d0, Dg))
            return out
        loop_ms, tables = events(loop)
        agrees = all(bool(np.array_equal(o, null_obs[t])) and bool(np.array_equal(enrich.expected_fixed(c_, w), null_expq[t]))
                     for t, (o, _, c_) in enumerate(tables))
        host_ms = host_agrees = None
        if a.host_shifts > 0:
            t0 = time.perf_counter()
            host_agrees = True
            for t in range(a.host_shifts):
                o = np.zeros((P, K), dtype=np.int64)
                cat = np.zeros((Dg, P), dtype=np.int64)
                for row, rng in zip(lv, ranges):
                    if rng is None:
                        continue
                    lo, hi, H, W, s1, s2, diag, chrom = region(row)
                    cls, seg = (np.roll(x, -int(shifts[chrom][t])) for x in ann[chrom])
                    ho, _, hc = host_tables(sv[lo:hi], H, W, diag, s2 - s1, K, cls[s1:s1 + H], cls[s2:s2 + W], seg[s1:s1 + H],
                                            seg[s2:s2 + W], d_min, d_max, rng[0], rng[1], a.chunk)
                    o += ho
                    cat[rng[0] - d0:rng[0] - d0 + rng[1]] += hc
                host_agrees = host_agrees and bool(np.array_equal(o, null_obs[t])) and \
                    bool(np.array_equal(enrich.expected_fixed(cat, w), null_expq[t]))
            host_ms = 1e3 * (time.perf_counter() - t0) / a.host_shifts * T
        loop_scaled = loop_ms / a.base_shifts * T
        res = dict(window=[d_min, d_max], nodes_inside=nodes, category_updates=nodes * T, shifts=T, null_ms=round(null_ms, 2),
                   loop_ms_per_shift=round(loop_ms / a.base_shifts, 3), loop_ms_scaled=round(loop_scaled, 1),
                   loop_over_null=round(loop_scaled / null_ms, 2), loop_agrees=agrees,
                   host_ms_per_shift=None if host_ms is None else round(host_ms / T, 1),
                   host_ms_scaled=None if host_ms is None else round(host_ms, 0),
                   host_over_null=None if host_ms is None else round(host_ms / null_ms, 1), host_agrees=host_agrees)
        print("%s: %s" % (label, json.dumps(res)), flush=True)
        return res

    out = dict(workload=a.workload, desc=desc, noise=a.noise, nodes=int(sv.size), blocks=int(lv.shape[0]), K=K, C=C, shifts=T,
               min_shift=a.min_shift, group=enrich.null_group(K, C), repeats=a.repeats, base_shifts=a.base_shifts,
               host_shifts=a.host_shifts, host_threads=min(16, os.cpu_count() or 1), windows={})
    out["windows"]["unlimited"] = run("unlimited", 0, -1)
    out["windows"]["window_%d" % a.window] = run("window_%d" % a.window, 0, a.window)
    out["not_measured"] = NOT_MEASURED
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
