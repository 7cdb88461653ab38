#!/usr/bin/env python3
"""Time the ancestral reconstruction on a synthetic workload (default cfg3: whole genome at 50 kb, 88.8 M nodes, K = 20,
S = 4, the example tree's A = 4 internal nodes), block by block as tools/segment_time.py does: device-resident
observations, the stencil graph built on the device, the generating model, then emission, a cold solve from argmax, and
on the resulting labels

    summary    phmrf_posterior_summary (conf, top): the yardstick -- the stage that exists since segmenting with a saved
               model, on the same logprob and labels
    ancestral  phmrf_ancestral in three forms: posterior weighting with sd, without sd, called weighting with sd

Per stage, summed over the blocks in milliseconds: the call as the host sees it (tables up, kernel, planes down), the
kernel alone (HIP events of the block's timing class posterior_stats) and a copy of the same number of bytes from a device
buffer into fresh pageable host memory, timed alone.  Per kernel the algorithmic bytes per node
  summary    4 K (logprob) + 1 (own label) + 5 (conf, top)
  posterior  4 K (logprob) + 4 S (observations) + 1 (own label) + 4 A (8 A with sd)
  called     4 S + 1 + 4 A (8 A with sd)
(+ 16 of the stencil's forward-edge weights per node on grid blocks for the first two, listed separately; the neighbours'
labels are other nodes' own labels and hit the cache) and the share of the 8 TB/s HBM peak they amount to.  One JSON
object, printed and written to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12                # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--beta1", type=float, default=0.5)
    ap.add_argument("--energy_tol_ppb", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ancestral_time.json"))
    a = ap.parse_args()
    import torch
    from phylo_hmrf_amd import Block, synthetic, workloads
    from phylo_hmrf_amd.tree import PhyloTree
    blocks, S, K, nn, desc = workloads.workload(a.workload)
    rng = np.random.default_rng(a.seed)
    tree = PhyloTree(synthetic.tree_for(S))
    params = synthetic.sample_ou_params(rng, tree, K)
    means, covars = tree.mean_cov(params, 2e-3)
    affine, cond_var = tree.ancestral_tables(params, 2e-3)
    A = affine.shape[1]
    dev = torch.device("cuda", 0)
    forms = dict(posterior_sd=("posterior", True), posterior=("posterior", False), called_sd=("called", True))
    call = dict(emission=0.0, solve=0.0, summary=0.0, **{f: 0.0 for f in forms})
    kernel = dict(summary=0.0, **{f: 0.0 for f in forms})
    d2h = dict(summary=0.0, planes=0.0, planes_sd=0.0)
    n_all, mean_sum = 0, 0.0

    def copy_alone(nbytes):
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        buf.cpu()
        return time.perf_counter() - t0

    for bi, (H, W, diag) in enumerate(blocks):
        n = workloads.block_nodes(H, W, diag)
        Xd = synthetic.device_observations(torch, dev, a.seed * 1000 + bi, H, W, diag, K, means, covars)
        torch.cuda.synchronize()
        b = Block(n, S, K)
        b.set_observations_dev(Xd.data_ptr())
        b.sync()
        b.build_grid_graph(H, W, diag, nn, a.beta1)
        b.sync()
        t0 = time.perf_counter()
        b.emission(means, covars)
        b.sync()
        t1 = time.perf_counter()
        b.solve_fast(a.beta, init_mode=1, energy_tol_ppb=a.energy_tol_ppb)
        t2 = time.perf_counter()
        b.enable_timing(True, classes=["posterior_stats"])
        b.reset_timing()
        b.posterior_summary(a.beta, 0)
        t3 = time.perf_counter()
        kernel["summary"] += b.timing()["posterior_stats"][0]
        call["emission"] += 1e3 * (t1 - t0)
        call["solve"] += 1e3 * (t2 - t1)
        call["summary"] += 1e3 * (t3 - t2)
        for f, (weighting, want_sd) in forms.items():
            b.reset_timing()
            t0 = time.perf_counter()
            mean, _ = b.ancestral(a.beta, 0, affine, cond_var, weighting, want_sd)
            call[f] += 1e3 * (time.perf_counter() - t0)
            ms, launches = b.timing()["posterior_stats"]
            assert launches == 1
            kernel[f] += ms
        b.enable_timing(False)
        mean_sum += float(mean.astype(np.float64).sum())
        d2h["summary"] += 1e3 * copy_alone(5 * n)
        d2h["planes"] += 1e3 * copy_alone(4 * A * n)
        d2h["planes_sd"] += 1e3 * copy_alone(8 * A * n)
        n_all += n
        del Xd
        b.close()
        torch.cuda.empty_cache()

    per_node = dict(summary=4 * K + 1 + 5, posterior_sd=4 * K + 4 * S + 1 + 8 * A, posterior=4 * K + 4 * S + 1 + 4 * A,
                    called_sd=4 * S + 1 + 8 * A)
    share = {f: per_node[f] * n_all / (kernel[f] * 1e-3) / HBM_PEAK for f in per_node}
    out = dict(workload=a.workload, desc=desc, nodes=n_all, blocks=len(blocks), K=K, S=S, A=A,
               call_ms={k: round(v, 2) for k, v in call.items()}, kernel_ms={k: round(v, 3) for k, v in kernel.items()},
               d2h_ms={k: round(v, 2) for k, v in d2h.items()}, bytes_per_node=per_node, forward_weight_bytes_per_node=16,
               hbm_share={k: round(v, 4) for k, v in share.items()}, mean_of_planes=mean_sum / max(A * n_all, 1))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
