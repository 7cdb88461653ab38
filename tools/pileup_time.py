#!/usr/bin/env python3
"""Time the pile-up of a state map around anchors (phmrf_state_pileup) on tools/enrich_time.py's genome map (default cfg3:
whole genome at 50 kb, 26 blocks, 88.8 M nodes, K = 20) with two anchor lists:

    anchors  on the diagonal, one every --every (20) bins of every chromosome, with controls --shift (50) bins along the
             diagonal to either side (with_controls): two groups
    pairs    --pairs (50,000) seeded anchor pairs, spread over the chromosomes by their bins, the two anchors 2 .. 40 bins
             apart: one group

both with a flank of --flank (20) bins, so 41 x 41 pile cells.  The map and every region's centres (region_centres: local
coordinates, mirror images for the off-diagonal blocks, culled, in group order) are on the GPU before anything is timed.
Per call, summed over the blocks, in milliseconds by HIP events around the library call (each call allocates and zeroes its
table, runs its kernel and copies the table to the host before it returns), the fastest of --repeats.  Beside it the host's
time on this machine for the same table: NumPy gathers over [centres, 41, 41] index arrays, --chunk centres at a time, and one
np.bincount, which must give an equal table.
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
NOT_MEASURED = ["the kernel's own time (no kernel trace was taken) and the share of the call that is allocation, the memset, the "
                "copy of the table and waits", "bytes moved and the share of the HBM peak",
                "state_pileup / pileup_files end to end (host -> device, the readers, the sum over regions, the text, the images)",
                "other K than the workload's 20, other flanks than --flank, more than two groups",
                "other tile, chunk and batch sizes of the kernel than the ones compiled in, and 32-bit counters in place of the packed ones",
                "the spread between runs (the fastest of --repeats counts)"]


def host_table(labels, H, W, diag, K, w, G, offsets, ci, cj, orient, chunk):
    """-> obs int64 [G, 2w + 1, 2w + 1, K] by NumPy, from the stored nodes"""
    side = 2 * w + 1
    S = side * side
    out = np.zeros(G * S * K, dtype=np.int64)
    u, v = np.arange(-w, w + 1, dtype=np.int64)[None, :, None], np.arange(-w, w + 1, dtype=np.int64)[None, None, :]
    cell = (np.arange(S, dtype=np.int64).reshape(1, side, side))
    grp = np.repeat(np.arange(G, dtype=np.int64), np.diff(offsets))
    for a in range(0, ci.shape[0], chunk):
        b = min(ci.shape[0], a + chunk)
        o = orient[a:b].astype(np.int64)[:, None, None]
        s = 1 - 2 * (o & 1)
        i = ci[a:b].astype(np.int64)[:, None, None] + s * np.where(o & 2, v, u)
        j = cj[a:b].astype(np.int64)[:, None, None] + s * np.where(o & 2, u, v)
        ok = (i >= 0) & (i < H) & (j >= 0) & (j < W)
        i, j = i[ok], j[ok]
        if diag:
            i, j = np.minimum(i, j), np.maximum(i, j)
            node = i * W - (i * (i - 1)) // 2 + (j - i)
        else:
            node = i * W + j
        where = np.broadcast_to(grp[a:b, None, None] * S + cell, ok.shape)[ok]
        out += np.bincount(where * K + labels[node], minlength=G * S * K)
    return out.reshape(G, side, side, K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--flank", type=int, default=20, help="bins to either side of a centre")
    ap.add_argument("--every", type=int, default=20, help="anchors: one every this many bins")
    ap.add_argument("--shift", type=int, default=50, help="anchors: the controls' shift in bins")
    ap.add_argument("--pairs", type=int, default=50000, help="pairs: how many")
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of every call; the fastest counts")
    ap.add_argument("--chunk", type=int, default=512, help="centres the host's restatement takes at a time")
    ap.add_argument("--no-host", action="store_true", help="leave the host's restatement out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup_time.json"))
    a = ap.parse_args()
    import torch
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib, pileup
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    w = a.flank
    side = 2 * w + 1

    def call(m_t, row, K, G, offsets, dev_arrays):
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        obs = np.zeros((G, side, side, K), dtype=np.int64)
        _lib.check(L.phmrf_state_pileup(ctypes.c_void_p(m_t[lo:hi].data_ptr()), H, W, diag, K, w, G, _lib.ptr_i64(offsets),
                                        *(ctypes.c_void_p(x.data_ptr()) for x in dev_arrays), _lib.ptr_i64(obs), st))
        return obs

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

    def run(name, m_t, sv, lv, K, centres, G):
        ms = host_ms = 0.0
        agree, submitted, calls, counted = True, 0, 0, 0
        for row in lv:
            offsets, ci, cj, ori = pileup.region_centres(centres, row, w, G)
            if not offsets[G]:
                continue
            dev_arrays = [torch.from_numpy(x).to(dev) for x in (ci, cj, ori)]
            t, got = timed(lambda: call(m_t, row, K, G, offsets, dev_arrays))
            ms += t
            calls += 1
            submitted += int(offsets[G])
            counted += int(got.sum())
            if not a.no_host:
                H, W, diag = (int(row[k]) for k in (3, 4, 8))
                t0 = time.perf_counter()
                want = host_table(sv[int(row[1]):int(row[2])], H, W, diag, K, w, G, offsets, ci, cj, ori, a.chunk)
                host_ms += 1e3 * (time.perf_counter() - t0)
                agree = agree and bool(np.array_equal(got, want))
        res = dict(centres=int(centres.shape[0]), groups=G, flank=w, pile_cells=side * side, calls=calls, centres_submitted=submitted,
                   cells_counted=counted, ms=round(ms, 3), host_ms=None if a.no_host else round(host_ms, 1),
                   host_agrees=None if a.no_host else agree, host_over_device=None if a.no_host else round(host_ms / ms, 1))
        print("%s: %s" % (name, json.dumps(res)), flush=True)
        if not a.no_host:
            assert agree, "%s: the host's table differs from the device's" % name
        return res

    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    print("genome maps ready: %d nodes" % sv.size, flush=True)
    m_t = torch.from_numpy(sv).to(dev)
    chroms = [int(c) for c in np.unique(lv[:, 9])]
    bins = {c: max(max(int(r[5] + r[3]), int(r[6] + r[4])) for r in lv if r[9] == c) for c in chroms}
    on_diagonal = np.concatenate([np.stack([np.full(len(x), c), x, x, 0 * x, 0 * x], axis=1)
                                  for c in chroms for x in [np.arange(a.every // 2, bins[c], a.every, dtype=np.int64)]])
    anchors = pileup.with_controls(on_diagonal, a.shift, 1)
    rng = np.random.default_rng(a.seed + 7)
    total = sum(bins.values())
    chrom = rng.choice(chroms, size=a.pairs, p=[bins[c] / total for c in chroms])
    span = np.array([bins[int(c)] for c in chrom])
    first = (rng.random(a.pairs) * (span - 41)).astype(np.int64)
    pairs = np.stack([chrom, first, first + rng.integers(2, 41, a.pairs), np.zeros(a.pairs, dtype=np.int64),
                      np.zeros(a.pairs, dtype=np.int64)], axis=1).astype(np.int64)
    # (code objects loaded before the first timing)
    offsets, ci, cj, ori = pileup.region_centres(anchors, lv[-1], w, 2)
    call(m_t, lv[-1], K, 2, offsets, [torch.from_numpy(x).to(dev) for x in (ci, cj, ori)])
    out = dict(repeats=a.repeats, host_threads=min(16, os.cpu_count() or 1), workload=a.workload, desc=desc, noise=a.noise,
               nodes=int(sv.size), blocks=int(lv.shape[0]), K=K, inputs={})
    out["inputs"]["anchors"] = dict(run("anchors", m_t, sv, lv, K, anchors, 2), every=a.every, shift=a.shift)
    out["inputs"]["pairs"] = dict(run("pairs", m_t, sv, lv, K, pairs, 1), distance=[2, 40])
    out["not_measured"] = NOT_MEASURED
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
