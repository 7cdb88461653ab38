#!/usr/bin/env python3
"""Time the interval-pair query of a state map (phmrf_rect_states through phylo_hmrf_amd.query's rectangles) on
tools/enrich_time.py's genome map (default cfg3: whole genome at 50 kb, 26 blocks, 88.8 M nodes, K = 20) with three lists:

    loops       --loops (default 50,000) seeded loops over the whole genome: two anchors of 1 .. 3 bins, 2 .. 40 bins apart,
                each with its two controls --shift (default 10) bins along the diagonal
    tad_pairs   every chromosome cut into consecutive intervals of 10 .. 40 bins; every pair of intervals (an interval with
                itself too) whose starts are at most 40 bins = 2 Mb apart
    big_pairs   the first chromosome's block cut into consecutive intervals of 100 .. 500 bins; every pair of them

The map is on the GPU and the rectangles of every region are made (query.rectangles, host) before anything is timed.  Per
list, in milliseconds by HIP events around the calls of all regions (query.region_states: each call clips and cuts its rectangles on the host,
uploads the item table, allocates and zeroes its tables, runs its kernel and copies the tables to the host before it
returns), the fastest of --repeats.  Beside it the host's time on this machine for the same tables from the same rectangles:
np.bincount over every rectangle's slice of the region's full matrix (a diagonal region's cells below the diagonal hold an
extra state that is dropped; the matrices are built outside the host's time), which must give equal tables.
One JSON object, printed and written to --out.
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
NOT_MEASURED = ["the kernel's own time apart from the call's fixed cost (clipping and cutting on the host, the upload of the item "
                "table, allocation, copies and waits): no kernel trace was taken", "bytes moved and the share of the HBM peak",
                "other item sizes than 16 x 256, another threshold of the word path than 32 columns, other grids",
                "holding a wave's histogram across the consecutive items of one rectangle",
                "state_query / query_files end to end (host -> device, the rectangles, the sum over regions, the text)",
                "confidence sums", "other K than the workload's 20", "the spread between runs (the fastest of --repeats counts)"]


def chrom_bins(lv):
    return {int(c): max(max(int(r[5] + r[3]), int(r[6] + r[4])) for r in lv if r[9] == c) for c in np.unique(lv[:, 9])}


def loops(bins, count, seed):
    rng = np.random.default_rng(seed)
    chroms = np.array(sorted(bins))
    c = rng.choice(chroms, count, p=np.array([bins[int(x)] for x in chroms]) / float(sum(bins.values())))
    size = np.array([bins[int(x)] for x in c])
    a0 = (rng.random(count) * (size - 50)).astype(np.int64)
    b0 = a0 + rng.integers(2, 41, count)
    return np.stack([c, a0, a0 + rng.integers(1, 4, count), b0, b0 + rng.integers(1, 4, count)], axis=1).astype(np.int64)


def interval_pairs(bins, lo, hi, reach, seed, chroms=None):
    """consecutive intervals of lo .. hi bins per chromosome; the pairs (t, u >= t) whose starts are at most `reach` bins
    apart (None: every pair)"""
    rng = np.random.default_rng(seed)
    rows = []
    for c in sorted(bins) if chroms is None else chroms:
        cuts = np.concatenate([[0], np.cumsum(rng.integers(lo, hi + 1, bins[c] // lo + 1))])
        cuts = cuts[cuts <= bins[c]]
        for t in range(len(cuts) - 1):
            for u in range(t, len(cuts) - 1):
                if reach is not None and cuts[u] - cuts[t] > reach:
                    break
                rows.append([c, cuts[t], cuts[t + 1], cuts[u], cuts[u + 1]])
    return np.array(rows, dtype=np.int64).reshape(-1, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--loops", type=int, default=50000)
    ap.add_argument("--shift", type=int, default=10, help="the loops' controls: this many bins along the diagonal")
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of every list; the fastest counts")
    ap.add_argument("--no-host", action="store_true", help="leave the host's restatement out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_time.json"))
    a = ap.parse_args()
    import torch
    from render_time import full_matrix
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib, query
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    print("genome maps ready: %d nodes" % sv.size, flush=True)
    m_t = torch.from_numpy(sv).to(dev)
    bins = chrom_bins(lv)
    mats = {}

    def device_tables(work, Q):
        total = np.zeros((Q, K), dtype=np.int64)
        for row, (rect, slot, minus) in zip(lv, work):
            if not rect.shape[0]:
                continue
            rows, part, _ = query.region_states(L, st, ctypes.c_void_p(m_t[int(row[1]):int(row[2])].data_ptr()), None, int(row[3]),
                                                int(row[4]), int(row[8]), K, rect, slot, minus)
            total[rows] += part
        return total

    def host_tables(work, Q):
        total = np.zeros((Q, K), dtype=np.int64)
        for row, (rect, slot, minus) in zip(lv, work):
            if not rect.shape[0]:
                continue
            if int(row[7]) not in mats:                      # the region's full matrix, made once and outside the host's time
                H, W, diag = int(row[3]), int(row[4]), int(row[8])
                M = full_matrix(sv[int(row[1]):int(row[2])], H, W, diag).copy()
                if diag:
                    M[np.tri(H, k=-1, dtype=bool)] = K       # not stored: an extra state, dropped below
                mats[int(row[7])] = M
        t0 = time.perf_counter()
        for row, (rect, slot, minus) in zip(lv, work):
            if not rect.shape[0]:
                continue
            M = mats[int(row[7])]
            sign = 1 - 2 * minus.astype(np.int64)
            for t in range(rect.shape[0]):
                i0, i1, j0, j1 = rect[t]
                total[slot[t]] += sign[t] * np.bincount(M[i0:i1, j0:j1].reshape(-1), minlength=K + 1)[:K]
        return total, 1e3 * (time.perf_counter() - t0)

    def run(name, q):
        work = [tuple(np.ascontiguousarray(x) for x in w) for w in query.rectangles(q, lv)]
        Q = q.shape[0]
        device_tables(work, Q)                               # (code objects loaded, allocator warm before the first timing)
        best, got = None, None
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            got = device_tables(work, Q)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        host_ms = agree = None
        if not a.no_host:
            want, host_ms = host_tables(work, Q)
            agree = bool(np.array_equal(got, want))
        rects = int(sum(w[0].shape[0] for w in work))
        items = int(sum(int((-(-(w[0][:, 1] - w[0][:, 0]) // query.TILE_H) * -(-(w[0][:, 3] - w[0][:, 2]) // query.TILE_W)).sum()) for w in work))
        res = dict(queries=Q, rectangles=rects, items_at_most=items, calls=int(sum(1 for w in work if w[0].shape[0])),
                   pairs=int(query.n_pairs(q).sum()), nodes_counted=int(got.sum()), ms=round(best, 3),
                   host_ms=None if host_ms is None else round(host_ms, 1), host_agrees=agree,
                   host_over_device=None if host_ms is None else round(host_ms / best, 1))
        print("%s: %s" % (name, json.dumps(res)), flush=True)
        return res

    out = dict(repeats=a.repeats, host_threads=min(16, os.cpu_count() or 1), workload=a.workload, desc=desc, noise=a.noise,
               nodes=int(sv.size), blocks=int(lv.shape[0]), K=K, lists={})
    q = loops(bins, a.loops, a.seed + 1)
    ctl, _ = query.with_controls(q, a.shift)
    out["lists"]["loops"] = dict(run("loops", np.concatenate([q, ctl])), loops=a.loops, controls=int(ctl.shape[0]), shift=a.shift)
    out["lists"]["tad_pairs"] = dict(run("tad_pairs", interval_pairs(bins, 10, 40, 40, a.seed + 2)), interval_bins=[10, 40], reach_bins=40)
    first = int(lv[0][9])
    out["lists"]["big_pairs"] = dict(run("big_pairs", interval_pairs(bins, 100, 500, None, a.seed + 3, chroms=[first])),
                                     interval_bins=[100, 500], chromosome=first)
    out["not_measured"] = NOT_MEASURED
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
