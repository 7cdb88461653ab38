#!/usr/bin/env python3
"""Time the genome tracks of state maps (phmrf_state_tracks) on two inputs:

    genome   tools/compare_time.py's map A of a synthetic workload (default cfg3: whole genome at 50 kb, 26 blocks, 88.8 M
             nodes, K = 20), every block with the unlimited window
    block    ONE diagonal block of the 10 kb workload's chr1 size (--block-side, default 24,895: 310 M stored nodes), a
             blocky map written straight into node order, with the unlimited window and with 0 .. --window (default 200) bins

The maps are on the GPU before anything is timed.  Per call, summed over the blocks, in milliseconds by HIP events around the
library call (each call allocates and zeroes its table, runs its kernel and copies the table to the host before it returns),
the fastest of --repeats.  Beside it the host's time on this machine for the same counts: the NumPy restatement on the full
matrix (np.bincount of row K + state over the cells inside the window, 512 matrix rows at a time), which is also checked
against the GPU's counts.  `window_over_unlimited` is the block's time with the window over its time without: far below 1
when the tiles outside the window are skipped.
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
NOT_MEASURED = ["the kernel's own time (no kernel trace was taken) and the share of the call that is allocation, copies and waits",
                "bytes moved and the share of the HBM peak", "state_tracks / tracks_files end to end (host -> device, the merge, the text)",
                "other K than the workload's, other windows than the two", "random maps (the row counts' runs are shortest there)",
                "the spread between runs (the fastest of --repeats counts)"]
CHUNK = 512


def host_tracks(M, K, dist0, d_min, d_max, want_cols):
    """-> (rows [H, K], cols [W, K] or None) of the full matrix M by NumPy"""
    H, W = M.shape
    rows = np.zeros((H, K), dtype=np.int64)
    cols = np.zeros(W * K, dtype=np.int64) if want_cols else None
    jj = np.arange(W, dtype=np.int64)[None, :]
    for a in range(0, H, CHUNK):
        b = min(H, a + CHUNK)
        part = M[a:b].astype(np.int64)
        ii = np.arange(a, b, dtype=np.int64)[:, None]
        if (d_min, d_max) == (0, -1):
            rows[a:b] = np.bincount((part + K * (ii - a)).reshape(-1), minlength=(b - a) * K).reshape(b - a, K)
            if want_cols:
                cols += np.bincount((part + K * jj).reshape(-1), minlength=W * K)
            continue
        d = np.abs(dist0 + jj - ii)
        ok = (d >= d_min) & ((d <= d_max) if d_max != -1 else True)
        rows[a:b] = np.bincount((part + K * (ii - a))[ok], minlength=(b - a) * K).reshape(b - a, K)
        if want_cols:
            cols += np.bincount((part + K * jj)[ok], minlength=W * K)
    return rows, (cols.reshape(W, K) if want_cols else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--block-side", type=int, default=24895, help="side of the single diagonal block (0: leave it out)")
    ap.add_argument("--window", type=int, default=200, help="the block's second window: 0 .. this many bins")
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of every call; the fastest counts")
    ap.add_argument("--no-host", action="store_true", help="leave the host's restatement out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_time.json"))
    a = ap.parse_args()
    import torch
    from render_time import blocky_nodes, full_matrix
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(m_t, row, K, d_min, d_max):
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        rows = np.zeros((H, K), dtype=np.int64)
        cols = None if diag else np.zeros((W, K), dtype=np.int64)
        _lib.check(L.phmrf_state_tracks(ctypes.c_void_p(m_t[lo:hi].data_ptr()), H, W, diag, int(row[6]) - int(row[5]), K, d_min,
                                        d_max, _lib.ptr_i64(rows), None if diag else _lib.ptr_i64(cols), st))
        return rows, cols

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

    def run(name, sv, lv, K, windows):
        m_t = torch.from_numpy(sv).to(dev)
        call(m_t, lv[-1], K, 0, 0)                           # (code objects loaded before the first timing)
        res = dict(nodes=int(sv.size), blocks=int(lv.shape[0]), K=K)
        for label, (d_min, d_max) in windows:
            ms = host_ms = 0.0
            agree, cells = True, 0
            for row in lv:
                H, W, diag = int(row[3]), int(row[4]), int(row[8])
                t, (rows, cols) = timed(lambda: call(m_t, row, K, d_min, d_max))
                ms += t
                cells += int(rows.sum())
                if not a.no_host:
                    M = full_matrix(sv[int(row[1]):int(row[2])], H, W, diag)
                    t0 = time.perf_counter()
                    want = host_tracks(M, K, int(row[6]) - int(row[5]), d_min, d_max, not diag)
                    host_ms += 1e3 * (time.perf_counter() - t0)
                    agree = agree and bool(np.array_equal(want[0], rows)) and (bool(diag) or bool(np.array_equal(want[1], cols)))
                    del M
            res[label] = dict(ms=round(ms, 3), window=[d_min, d_max], cells_inside=cells,
                              host_ms=None if a.no_host else round(host_ms, 1), host_agrees=None if a.no_host else agree)
            print("%s %s: %s" % (name, label, json.dumps(res[label])), flush=True)
        del m_t
        return res

    out = dict(repeats=a.repeats, host_threads=min(16, os.cpu_count() or 1), inputs={})
    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    print("genome maps ready: %d nodes" % sv.size, flush=True)
    out["inputs"]["genome"] = dict(run("genome", sv, lv, K, (("unlimited", (0, -1)),)), workload=a.workload, desc=desc,
                                   noise=a.noise)
    del sv
    if a.block_side > 0:
        side = a.block_side
        n = side * (side + 1) // 2
        sv = blocky_nodes(side, K, a.seed + 1)
        print("block ready: %d nodes" % sv.size, flush=True)
        lv = np.array([[n, 0, n, side, side, 0, 0, 0, 1, 1]], dtype=np.int64)
        res = run("block", sv, lv, K, (("unlimited", (0, -1)), ("window_%d" % a.window, (0, a.window))))
        out["inputs"]["block"] = dict(res, block_side=side)
        out["window_over_unlimited"] = round(res["window_%d" % a.window]["ms"] / res["unlimited"]["ms"], 4)
    out["not_measured"] = NOT_MEASURED
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
