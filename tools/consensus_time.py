#!/usr/bin/env python3
"""Time the consensus of M state maps (phmrf_label_consensus) on a synthetic workload's label maps (default cfg3: whole
genome at 50 kb, 26 blocks, 88.8 M nodes, K = 20): tools/smooth_time.py's blocky map without its noise, and M copies of it
(default M = 3 and M = 8) with --noise of their nodes redrawn, each copy by its own generator.

The maps are on the GPU before anything is timed.  Per M, summed over the blocks, in milliseconds by HIP events around the
library call (each call allocates and zeroes its tables, checks the labels, votes and copies the tables to the host before it
returns), the fastest of --repeats; the planes consensus, support and core are all written.  With it the bytes the vote has
to move, (M + 3) n -- every map read once, three planes written --, the rate that amounts to against the 8 TB/s HBM peak, and
the same with the check pass's second reading of the maps counted in.  Beside it the host's time on this machine for the same
answers by NumPy (one-hot vote planes, argmax, np.bincount of index arrays, the bands from the coordinate arrays), which is
also checked against the GPU's planes and tables.
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
HBM_PEAK = 8e12                # bytes / s
BANDS = 32
NOT_MEASURED = ["the kernels' own time apart from the call's fixed cost (two allocations, two memsets, the check's flag and the "
                "tables' copy to the host with their two waits): no kernel trace was taken, and the check pass is not separated "
                "from the vote", "consensus_states / consensus_files end to end (host -> device, the matching, the text, the .mat)",
                "other K than the workload's, K > 22 at M = 16 where agree goes through the chunk kernel", "a renumbering table",
                "random maps (the shortest runs of equal key)", "the spread between runs (the fastest of --repeats counts)"]


def host_consensus(S, K, min_support, H, W, diag, dist0):
    """-> (consensus, support, core, support_hist, agree, pair, bands) of one region's maps S [M, n] by NumPy"""
    M, n = S.shape
    votes = np.zeros((K, n), dtype=np.uint8)
    at = np.arange(n)
    for m in range(M):
        votes[S[m], at] += 1
    cons = votes.argmax(axis=0)
    support = votes[cons, at].astype(np.int64)
    del votes
    core = np.where(support >= min_support, cons, K)
    hist = np.bincount(cons * (M + 1) + support, minlength=K * (M + 1)).reshape(K, M + 1)
    agree = np.stack([np.bincount(cons * K + S[m], minlength=K * K).reshape(K, K) for m in range(M)])
    pair = np.array([[n if a == b else int(np.count_nonzero(S[a] == S[b])) for b in range(M)] for a in range(M)], dtype=np.int64)
    ii, jj = np.triu_indices(H) if diag else np.divmod(at, W)
    band = np.searchsorted(2 ** np.arange(BANDS, dtype=np.int64), np.abs(dist0 + jj.astype(np.int64) - ii), side="right")
    bands = np.stack([np.bincount(band, minlength=BANDS), np.bincount(band[support >= min_support], minlength=BANDS),
                      np.bincount(band[support == M], minlength=BANDS)], axis=1)
    return cons, support, core, hist, agree, pair, bands


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1, help="the share of its nodes every copy redraws")
    ap.add_argument("--maps", default="3,8", help="the numbers of maps to time")
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of every call; the fastest counts")
    ap.add_argument("--no-host", action="store_true", help="leave the host's restatement out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_time.json"))
    a = ap.parse_args()
    import torch
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    counts = [int(x) for x in a.maps.split(",")]
    truth, lv, K, desc = genome_maps(a.workload, a.seed, 0.0)
    n = int(truth.size)
    print("blocky map ready: %d nodes, %d blocks" % (n, lv.shape[0]), flush=True)
    copies = np.empty((max(counts), n), dtype=np.uint8)
    for m in range(max(counts)):
        rng = np.random.default_rng([a.seed, m + 1])
        copies[m] = truth
        hit = rng.random(n) < a.noise
        copies[m, hit] = rng.integers(0, K, int(hit.sum()), dtype=np.uint8)
    del truth
    S_t = torch.from_numpy(copies).to(dev)
    planes = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(3)]

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

    def call(M, row, min_support):
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        ptrs = (ctypes.c_void_p * M)(*[S_t[m, lo:hi].data_ptr() for m in range(M)])
        hist, agree = np.zeros((K, M + 1), dtype=np.int64), np.zeros((M, K, K), dtype=np.int64)
        pair, bands = np.zeros((M, M), dtype=np.int64), np.zeros((BANDS, 3), dtype=np.int64)
        _lib.check(L.phmrf_label_consensus(ctypes.cast(ptrs, ctypes.c_void_p), M, None, K, H, W, diag, int(row[6]) - int(row[5]),
                                           min_support, *[ctypes.c_void_p(p[lo:hi].data_ptr()) for p in planes],
                                           _lib.ptr_i64(hist), _lib.ptr_i64(agree), _lib.ptr_i64(pair), _lib.ptr_i64(bands), st))
        return hist, agree, pair, bands

    call(counts[0], lv[-1], 1)                               # (code objects loaded before the first timing)
    out = dict(workload=a.workload, desc=desc, nodes=n, blocks=int(lv.shape[0]), K=K, noise=a.noise, repeats=a.repeats,
               host_threads=min(16, os.cpu_count() or 1), maps={})
    for M in counts:
        ms_need = M // 2 + 1
        ms = host_ms = 0.0
        agrees, stable, unanimous = True, 0, 0
        for row in lv:
            lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
            t, (hist, agree, pair, bands) = timed(lambda: call(M, row, ms_need))
            ms += t
            stable += int(bands[:, 1].sum())
            unanimous += int(bands[:, 2].sum())
            if not a.no_host:
                S = copies[:M, lo:hi].astype(np.int64)
                t0 = time.perf_counter()
                want = host_consensus(S, K, ms_need, H, W, diag, int(row[6]) - int(row[5]))
                host_ms += 1e3 * (time.perf_counter() - t0)
                got = [p[lo:hi].cpu().numpy() for p in planes] + [hist, agree, pair, bands]
                agrees = agrees and all(bool(np.array_equal(g, w)) for g, w in zip(got, want))
                del S, want, got
        vote_bytes, with_check = (M + 3) * n, (2 * M + 3) * n
        res = dict(ms=round(ms, 3), min_support=ms_need, stable_share=round(stable / n, 4), unanimous_share=round(unanimous / n, 4),
                   vote_bytes=vote_bytes, vote_gb_per_s=round(vote_bytes / ms / 1e6, 1),
                   vote_share_of_hbm_peak=round(vote_bytes / (ms * 1e-3) / HBM_PEAK, 4),
                   bytes_with_check_pass=with_check, with_check_gb_per_s=round(with_check / ms / 1e6, 1),
                   with_check_share_of_hbm_peak=round(with_check / (ms * 1e-3) / HBM_PEAK, 4),
                   host_ms=None if a.no_host else round(host_ms, 1), host_agrees=None if a.no_host else agrees,
                   host_over_gpu=None if a.no_host else round(host_ms / ms, 1))
        out["maps"][str(M)] = res
        print("M = %d: %s" % (M, json.dumps(res)), flush=True)
    out["not_measured"] = NOT_MEASURED
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
