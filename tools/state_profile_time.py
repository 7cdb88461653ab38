#!/usr/bin/env python3
"""Time the state profile on a synthetic workload (default cfg3: whole genome at 50 kb, 26 blocks, 88.8 M nodes, K = 20,
S = 4) with the five default quantiles.  The labels are tools/smooth_time.py's maps (synthetic.label_image with
salt-and-pepper noise); the observations are a per-state mean vector plus normal noise, so that -- as in real data -- most
values of a state and species share the top byte of their key.  Observations and labels are on the GPU before anything is
timed.  Reported, in milliseconds:

    passes       per pass of the radix selection: its shift, J, the time of the phmrf_state_hist calls by HIP events around
                 the library call (each call allocates its scratch, runs its kernel and reads the histograms back), summed over
                 the blocks, and the bytes the pass moves: bytes_loaded = what the lanes load (S J workgroup rows, each the
                 labels and one species' values: 5 bytes per node), bytes_lines = the cache lines those loads touch (a
                 node's S values lie together: 1 + 4 S bytes per node and workgroup row), bytes_once = labels and
                 observations read once; hbm_share = bytes_loaded per second against the 8 TB/s peak
    moments      the phmrf_state_moments calls (counts, sums, sums of squares, bands) the same way
    first_two_over_last_two   time of the passes at shift 24 and 16 over that of the passes at 8 and 0, per byte loaded:
                 what the concentration of the data in few bins costs after the aggregation
    state_profile   profile.state_profile end to end (wall clock), on a stand-in for the model that holds the blocks
    host         the same numbers on this machine's CPU with at most 16 threads: np.partition per (state, species) for the
                 order statistics, np.bincount with weights for the moments, over the same float32 data

One JSON object, printed and written to --out.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK = 8e12                # bytes / s


class HeldBlocks(object):
    """what profile.state_profile asks of a model, for blocks made here: whole blocks on one rank, no tiles"""

    def __init__(self, blocks, len_vec, K, S):
        from phylo_hmrf_amd.concurrent import BlockRunner
        from phylo_hmrf_amd.dist import Reducer
        self.blocks = dict(enumerate(blocks))
        self.len_vec = [list(map(int, lv)) for lv in len_vec]
        self.my_regions = list(self.blocks)
        self.general_graph_regions = []
        self.n_components, self.n_features = K, S
        self.n_samples = int(self.len_vec[-1][2])
        self.world, self.reducer, self.runner = 1, Reducer(1), BlockRunner(1)

        class _NoTiles(object):
            groups = []
        self.conductor = _NoTiles()


def stage(text):
    print("[state_profile_time] %s" % text, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--spread", type=float, default=0.3, help="sd of the observations around their state's mean")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_profile_time.json"))
    a = ap.parse_args()
    import torch
    from smooth_time import genome_maps
    from phylo_hmrf_amd import Block, _lib, profile
    from phylo_hmrf_amd import workloads
    stage("label maps of %s" % a.workload)
    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    S = int(workloads.workload(a.workload)[1])
    n = int(sv.size)
    rng = np.random.default_rng(a.seed + 2)
    mu = rng.uniform(0.5, 6.0, (K, S)).astype(np.float32)
    x32 = np.empty((n, S), dtype=np.float32)
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)          # the blocks run on it, the events are recorded on it
    stream = side.cuda_stream
    blocks = []
    for row in lv:
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        x32[lo:hi] = mu[sv[lo:hi]] + np.float32(a.spread) * rng.standard_normal((hi - lo, S), dtype=np.float32)
        b = Block(hi - lo, S, K)
        b.set_stream(stream)
        b.set_observations(x32[lo:hi].astype(np.float64))
        b.build_grid_graph(H, W, bool(diag), 8, 0.5)
        b.set_labels(sv[lo:hi])
        blocks.append(b)
        stage("block %d of %d on the device (%d nodes)" % (len(blocks), len(lv), hi - lo))
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        out = fn()
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    # the moments, then the selection pass by pass, each library call between two events
    ms_moments = 0.0
    count, total, sq = np.zeros(K, dtype=np.int64), np.zeros((K, S)), np.zeros((K, S))
    for b, row in zip(blocks, lv):
        ms, got = timed(lambda: b.state_moments(int(row[6]) - int(row[5]), want_bands=True))
        ms_moments += ms
        count, total, sq = count + got[0], total + got[1], sq + got[2]
    stage("moments %.1f ms" % ms_moments)
    passes = []

    def run_pass(shift, prefix):
        hist, ms_pass = 0, 0.0
        for b in blocks:
            ms, h = timed(lambda: b.state_hist(shift, prefix))
            ms_pass += ms
            hist = hist + h.astype(np.int64)
        J = int(prefix.shape[2])
        loaded = n * S * J * 5
        passes.append(dict(shift=shift, J=J, ms=round(ms_pass, 3), bytes_loaded=loaded, bytes_lines=n * S * J * (1 + 4 * S),
                           bytes_once=n * (1 + 4 * S), hbm_share=round(loaded / (ms_pass * 1e-3) / HBM_PEAK, 4)))
        stage("pass at shift %d, J = %d: %.1f ms" % (shift, J, ms_pass))
        return hist

    q = np.asarray(profile.DEFAULT_QUANTILES)
    lo_r, hi_r, _ = profile.quantile_ranks(count, q)
    ranks = np.broadcast_to(np.concatenate([lo_r, hi_r], axis=1)[:, None, :], (K, S, 2 * q.size))
    t0 = time.perf_counter()
    stat = profile.select(run_pass, lambda h: h, count, ranks)
    select_ms = 1e3 * (time.perf_counter() - t0)
    per_byte = [p["ms"] / p["bytes_loaded"] for p in passes]
    ratio = (per_byte[0] + per_byte[1]) / (per_byte[2] + per_byte[3])

    model = HeldBlocks(blocks, lv, K, S)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prof = profile.state_profile(model)
    whole_ms = 1e3 * (time.perf_counter() - t0)
    stage("state_profile %.1f ms; the host's turn" % whole_ms)
    assert np.array_equal(prof["count"], count)
    assert np.array_equal(np.concatenate([prof["q_lo"], prof["q_hi"]], axis=2).view(np.uint32), stat.view(np.uint32))
    for b in blocks:
        b.close()

    # the host's yardstick over the same float32 data: at most 16 threads
    threads = min(16, os.cpu_count() or 1)
    host = {}
    t0 = time.perf_counter()
    members = [np.flatnonzero(sv == k) for k in range(K)]
    host["gather_ms"] = 1e3 * (time.perf_counter() - t0)

    def order_stats(ks):
        k, s = ks
        if count[k] == 0:
            return np.full(2 * q.size, np.nan, dtype=np.float32)
        kth = np.unique(np.concatenate([lo_r[k], hi_r[k]]))
        v = np.partition(x32[members[k], s], kth)
        return v[np.concatenate([lo_r[k], hi_r[k]])]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        ref = np.stack(list(pool.map(order_stats, [(k, s) for k in range(K) for s in range(S)]))).reshape(K, S, 2 * q.size)
    host["partition_ms"] = 1e3 * (time.perf_counter() - t0)
    stage("host partition %.0f ms" % host["partition_ms"])
    assert np.array_equal(ref, stat, equal_nan=True)

    def host_moments(s):
        col = x32[:, s].astype(np.float64)
        return np.bincount(sv, weights=col, minlength=K), np.bincount(sv, weights=col * col, minlength=K)

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        hm = list(pool.map(host_moments, range(S)))
    ref_count = np.bincount(sv, minlength=K)
    host["moments_ms"] = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(ref_count, count)
    assert np.allclose(np.stack([h[0] for h in hm], axis=1), total, rtol=1e-9)

    out = dict(workload=a.workload, desc=desc, nodes=n, blocks=int(lv.shape[0]), K=K, S=S, noise=a.noise, spread=a.spread,
               quantiles=q.tolist(), passes=passes, select_ms=round(select_ms, 1),
               moments=dict(ms=round(ms_moments, 3), bytes_once=n * (1 + 4 * S),
                            hbm_share=round(n * (1 + 4 * S) / (ms_moments * 1e-3) / HBM_PEAK, 4)),
               first_two_over_last_two=round(ratio, 3), state_profile_ms=round(whole_ms, 1),
               state_profile_timing={k: (v if k == "passes" else round(v, 1)) for k, v in prof["timing"].items()},
               host_ms={k: round(v, 1) for k, v in host.items()}, host_threads=threads,
               not_measured="K = 64, S = 16; whether LDS atomics or the re-reads of the observations bound a pass")
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
