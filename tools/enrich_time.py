#!/usr/bin/env python3
"""Time the pair enrichment of state maps (phmrf_pair_enrichment) on two inputs:

    genome   tools/compare_time.py's map A of a synthetic workload (default cfg3: whole genome at 50 kb, 26 blocks, 88.8 M
             nodes, K = 20), every block with the unlimited window
    block    ONE diagonal block of the 10 kb workload's chr1 size (--block-side, default 24,895: 310 M stored nodes), a
             blocky map written straight into node order, with the window 0 .. --window (default 200) bins

The annotation: three classes (0: none) in intervals of 100 .. 500 bins along every chromosome, every interval a segment of its
own.  Maps and annotation are on the GPU before anything is timed.  Per call, summed over the blocks, in milliseconds by HIP
events around the library call (each call allocates and zeroes its three tables, runs its two kernels and copies the tables
to the host before it returns), the fastest of --repeats.  Beside it the host's time on this machine for the same three
tables: np.bincount over the index arrays of the stored nodes inside the window (as tests/enrich_reference.py, --chunk storage
rows at a time and only the columns the window reaches), which must give equal tables.
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
NOT_MEASURED = ["the two kernels' own time (no kernel trace was taken) and the share of the call that is allocation, copies and waits",
                "bytes moved and the share of the HBM peak", "pair_enrichment / enrich_files end to end (host -> device, the sum over "
                "regions, the expectation, the text)", "other K and C than the workload's 20 and 3, other windows than the two",
                "random maps and per-bin annotations (the runs of equal bins are shortest there)",
                "the spread between runs (the fastest of --repeats counts)"]
C = 3


def annotation(bins, seed):
    """-> (u8 classes [bins], int32 segments [bins]): intervals of 100 .. 500 bins, each a segment of its own"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(100, 501, bins // 100 + 1)
    return (np.repeat(rng.integers(0, C, lengths.shape[0]), lengths)[:bins].astype(np.uint8),
            np.repeat(np.arange(lengths.shape[0]), lengths)[:bins].astype(np.int32))


def host_tables(labels, H, W, diag, dist0, K, rc, cc, rs, cs, d_min, d_max, d_lo, D, chunk):
    """-> (obs [P, K], state_dist [D, K], cat_dist [D, P]) by NumPy"""
    P = 2 * C * C
    obs, sd, cd = np.zeros(P * K, dtype=np.int64), np.zeros(D * K, dtype=np.int64), np.zeros(D * P, dtype=np.int64)
    rc, cc, rs, cs = (np.asarray(x, dtype=np.int64) for x in (rc, cc, rs, cs))
    for a in range(0, H, chunk):
        b = min(H, a + chunk)
        j0, j1 = (a if diag else 0), W
        if d_max != -1:                                      # the columns with |dist0 + j - i| <= d_max for some row of the chunk
            j0, j1 = max(j0, a - dist0 - d_max), min(W, b - dist0 + d_max)
        if j1 <= j0:
            continue
        ii, jj = np.arange(a, b, dtype=np.int64)[:, None], np.arange(j0, j1, dtype=np.int64)[None, :]
        d = np.abs(dist0 + jj - ii)
        ok = (d >= d_min) & ((d <= d_max) if d_max != -1 else True)
        if diag:
            ok &= jj >= ii
        base = ii * W - (ii * (ii - 1)) // 2 - ii if diag else ii * W
        s = labels[(base + jj)[ok]].astype(np.int64)
        i_in, j_in = np.broadcast_to(ii, ok.shape)[ok], np.broadcast_to(jj, ok.shape)[ok]
        p = (rc[i_in] * C + cc[j_in]) * 2 + ((rs[i_in] >= 0) & (rs[i_in] == cs[j_in]))
        t = d[ok] - d_lo
        obs += np.bincount(p * K + s, minlength=P * K)
        sd += np.bincount(t * K + s, minlength=D * K)
        cd += np.bincount(t * P + p, minlength=D * P)
    return obs.reshape(P, K), sd.reshape(D, K), cd.reshape(D, P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--block-side", type=int, default=24895, help="side of the single diagonal block (0: leave it out)")
    ap.add_argument("--window", type=int, default=200, help="the block's window: 0 .. this many bins")
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of every call; the fastest counts")
    ap.add_argument("--chunk", type=int, default=256, help="storage rows the host's restatement takes at a time")
    ap.add_argument("--no-host", action="store_true", help="leave the host's restatement out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enrich_time.json"))
    a = ap.parse_args()
    import torch
    from render_time import blocky_nodes
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib, enrich
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = 2 * C * C

    def call(m_t, row, K, ann_t, d_min, d_max, d_lo, D):
        lo, hi, H, W, s1, s2, diag = (int(row[k]) for k in (1, 2, 3, 4, 5, 6, 8))
        cls_t, seg_t = ann_t
        obs, sd, cd = np.zeros((P, K), dtype=np.int64), np.zeros((D, K), dtype=np.int64), np.zeros((D, P), dtype=np.int64)
        _lib.check(L.phmrf_pair_enrichment(
            ctypes.c_void_p(m_t[lo:hi].data_ptr()), H, W, diag, s2 - s1, K, C, ctypes.c_void_p(cls_t[s1:].data_ptr()),
            ctypes.c_void_p(cls_t[s2:].data_ptr()), ctypes.c_void_p(seg_t[s1:].data_ptr()), ctypes.c_void_p(seg_t[s2:].data_ptr()),
            d_min, d_max, d_lo, D, _lib.ptr_i64(obs), _lib.ptr_i64(sd), _lib.ptr_i64(cd), st))
        return obs, sd, cd

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

    def run(name, sv, lv, K, label, d_min, d_max):
        m_t = torch.from_numpy(sv).to(dev)
        ann, ann_t = {}, {}
        for c in np.unique(lv[:, 9]):                        # one annotation per chromosome, the regions take slices of it
            bins = max(max(int(r[5] + r[3]), int(r[6] + r[4])) for r in lv if r[9] == c)
            ann[int(c)] = annotation(bins, a.seed + 100 + int(c))
            ann_t[int(c)] = tuple(torch.from_numpy(x).to(dev) for x in ann[int(c)])
        call(m_t, lv[-1], K, ann_t[int(lv[-1][9])], 0, 0, 0, 1)                 # (code objects loaded before the first timing)
        ms = host_ms = 0.0
        agree, nodes = True, 0
        for row in lv:
            H, W, s1, s2, diag, chrom = (int(row[k]) for k in (3, 4, 5, 6, 8, 9))
            rng = enrich.distance_range(H, W, diag, s2 - s1, d_min, d_max)
            if rng is None:
                continue
            t, got = timed(lambda: call(m_t, row, K, ann_t[chrom], d_min, d_max, rng[0], rng[1]))
            ms += t
            nodes += int(got[0].sum())
            if not a.no_host:
                cls, seg = ann[chrom]
                t0 = time.perf_counter()
                want = host_tables(sv[int(row[1]):int(row[2])], H, W, diag, s2 - s1, K, cls[s1:s1 + H], cls[s2:s2 + W], seg[s1:s1 + H],
                                   seg[s2:s2 + W], d_min, d_max, rng[0], rng[1], a.chunk)
                host_ms += 1e3 * (time.perf_counter() - t0)
                agree = agree and all(bool(np.array_equal(x, y)) for x, y in zip(got, want))
        res = dict(nodes=int(sv.size), blocks=int(lv.shape[0]), K=K, C=C, window=[d_min, d_max], nodes_inside=nodes,
                   ms=round(ms, 3), host_ms=None if a.no_host else round(host_ms, 1), host_agrees=None if a.no_host else agree,
                   host_over_device=None if a.no_host else round(host_ms / ms, 1))
        print("%s %s: %s" % (name, label, json.dumps(res)), flush=True)
        del m_t
        return res

    out = dict(repeats=a.repeats, host_threads=min(16, os.cpu_count() or 1), inputs={})
    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    print("genome maps ready: %d nodes" % sv.size, flush=True)
    out["inputs"]["genome"] = dict(run("genome", sv, lv, K, "unlimited", 0, -1), workload=a.workload, desc=desc, noise=a.noise)
    del sv
    if a.block_side > 0:
        side = a.block_side
        n = side * (side + 1) // 2
        sv = blocky_nodes(side, K, a.seed + 1)
        print("block ready: %d nodes" % sv.size, flush=True)
        lv = np.array([[n, 0, n, side, side, 0, 0, 0, 1, 1]], dtype=np.int64)
        out["inputs"]["block"] = dict(run("block", sv, lv, K, "window_%d" % a.window, 0, a.window), block_side=side)
    out["not_measured"] = NOT_MEASURED
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
