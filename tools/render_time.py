#!/usr/bin/env python3
"""Time the images of state maps (phmrf_render_states) on two inputs:

    genome   tools/compare_time.py's map A of a synthetic workload (default cfg3: whole genome at 50 kb, 26 blocks, 88.8 M
             nodes, K = 20), every block drawn at factor 1 and at --side (default 2048) pixels a side
    block    ONE diagonal block of the 10 kb workload's chr1 size (--block-side, default 24,895: 310 M stored nodes, labels
             only), a blocky map written straight into node order, drawn at --side pixels a side

The maps are on the GPU before anything is timed.  Per call, summed over the blocks, in milliseconds by HIP events around the
library call (each call allocates its planes, runs its two kernels and copies the planes and the image to the host before
it returns), the fastest of --repeats.  Beside it the host's time on this machine for the same state planes: a NumPy
block vote on the full matrix (per state, the cells of every pixel summed over the reshaped matrix; the lowest argmax), which
is also checked against the GPU's state plane.
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
NOT_MEASURED = ["the kernels' own time (no kernel trace was taken) and the share of the call that is allocation, copies and waits",
                "bytes moved and the share of the HBM peak", "maps with confidences or marks (labels only)",
                "render_states / render_files end to end (host -> device, the PNG writer)",
                "other K than the workload's, other factors than 1 and the --side one",
                "the spread between runs (the fastest of --repeats counts)"]


def blocky_nodes(side, K, seed, mean_run=40):
    """u8 labels of a diagonal block in node order: constant tiles of 1 .. 2 mean_run - 1 bins a side, symmetric by
    construction, written storage row by storage row (the full matrix is never built)"""
    rng = np.random.default_rng(seed)
    cuts = np.repeat(np.arange(side), rng.integers(1, 2 * mean_run, side))[:side]
    nt = int(cuts[-1]) + 1
    table = rng.integers(0, K, (nt, nt)).astype(np.uint8)
    table = np.triu(table) + np.triu(table, 1).T
    out = np.empty(side * (side + 1) // 2, dtype=np.uint8)
    at = 0
    for i in range(side):
        out[at:at + side - i] = table[cuts[i], cuts[i:]]
        at += side - i
    return out


def full_matrix(states, H, W, diag):
    """node order -> the H x W matrix, storage row by storage row (no index arrays: the 10 kb block has 310 M nodes)"""
    if not diag:
        return states.reshape(H, W)
    M = np.empty((H, H), dtype=states.dtype)
    at = 0
    for i in range(H):
        M[i, i:] = M[i:, i] = states[at:at + H - i]
        at += H - i
    return M


def host_vote(M, K, f):
    """-> the state plane of the full matrix M by NumPy: per state the pixels' counts, the lowest state of the largest"""
    H, W = M.shape
    h, w = -(-H // f), -(-W // f)
    P = np.full((h * f, w * f), 255, dtype=np.uint8)
    P[:H, :W] = M
    P = P.reshape(h, f, w, f)
    best = np.zeros((h, w), dtype=np.int64)
    state = np.zeros((h, w), dtype=np.uint8)
    for k in range(K):
        c = (P == k).sum(axis=(1, 3), dtype=np.int64)
        better = c > best
        best[better] = c[better]
        state[better] = k
    return state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--side", type=int, default=2048, help="the largest side of an image in pixels")
    ap.add_argument("--block-side", type=int, default=24895, help="side of the single diagonal block (0: leave it out)")
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of every call; the fastest counts")
    ap.add_argument("--no-host", action="store_true", help="leave the host's block vote out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.json"))
    a = ap.parse_args()
    import torch
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib, render
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    extra = np.array(render.HIGHLIGHT + render.OUTLINE, dtype=np.uint8)

    def call(m_t, row, K, f, pal):
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        h, w = -(-H // f), -(-W // f)
        planes, rgb = np.zeros((3, h, w), dtype=np.uint8), np.zeros((h, w, 3), dtype=np.uint8)
        _lib.check(L.phmrf_render_states(ctypes.c_void_p(m_t[lo:hi].data_ptr()), None, None, H, W, diag, K, f,
                                         pal.ctypes.data_as(ctypes.c_void_p), extra.ctypes.data_as(ctypes.c_void_p), 0,
                                         planes.ctypes.data_as(ctypes.c_void_p), rgb.ctypes.data_as(ctypes.c_void_p), st))
        return planes[0]

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

    def run(name, sv, lv, K, settings):
        """settings: (label, factor or None for choose_factor) -> the input's entry of the JSON"""
        pal = render.default_palette(K)
        m_t = torch.from_numpy(sv).to(dev)
        call(m_t, lv[-1], K, 1 if int(lv[-1][3]) <= 4096 else render.choose_factor(lv[-1][3], lv[-1][4], a.side), pal)
        res = dict(nodes=int(sv.size), blocks=int(lv.shape[0]), K=K)
        for label, fixed in settings:
            ms = host_ms = 0.0
            pixels, factors, agree = 0, [], True
            for row in lv:
                H, W, diag = int(row[3]), int(row[4]), int(row[8])
                f = fixed or render.choose_factor(H, W, a.side)
                t, state = timed(lambda: call(m_t, row, K, f, pal))
                ms += t
                pixels += state.size
                factors.append(f)
                if not a.no_host:
                    M = full_matrix(sv[int(row[1]):int(row[2])], H, W, diag)
                    t0 = time.perf_counter()
                    want = host_vote(M, K, f)
                    host_ms += 1e3 * (time.perf_counter() - t0)
                    agree = agree and bool(np.array_equal(want, state))
                    del M
            res[label] = dict(ms=round(ms, 3), pixels=pixels, factors=sorted(set(factors)),
                              host_ms=None if a.no_host else round(host_ms, 1), host_agrees=None if a.no_host else agree)
            print("%s %s: %s" % (name, label, json.dumps(res[label])), flush=True)
        del m_t
        return res

    out = dict(side=a.side, repeats=a.repeats, host_threads=min(16, os.cpu_count() or 1), inputs={})
    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    print("genome maps ready: %d nodes" % sv.size, flush=True)
    out["inputs"]["genome"] = dict(run("genome", sv, lv, K, (("factor_1", 1), ("side_%d" % a.side, None))), workload=a.workload,
                                   desc=desc, noise=a.noise)
    del sv
    if a.block_side > 0:
        side = a.block_side
        n = side * (side + 1) // 2
        sv = blocky_nodes(side, K, a.seed + 1)
        print("block ready: %d nodes" % sv.size, flush=True)
        lv = np.array([[n, 0, n, side, side, 0, 0, 0, 1, 1]], dtype=np.int64)
        out["inputs"]["block"] = dict(run("block", sv, lv, K, (("side_%d" % a.side, None),)), block_side=side)
    out["not_measured"] = NOT_MEASURED
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
