#!/usr/bin/env python3
"""Time a segmentation with a saved model, stage by stage, on a synthetic workload (default cfg3: whole genome at 50 kb,
88.8 M nodes, K = 20, S = 4).  The model is the generating one (OU parameters drawn as bench.py draws them, Gaussians +
min_covar I); every block gets device-resident observations and its stencil graph built on the device, then the three
steps of segment.py: emission, a cold solve from argmax_k logprob, the posterior summary.  Printed per stage, summed over
the blocks in milliseconds (each stage synchronised):

    emission | cold solve | summary (kernel + copy of conf / top to the host) | d2h (the same bytes copied alone)

The summary kernel's own time comes from a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/segment_time.py
(posterior_summary_kernel); its algorithmic bytes per node are 4 K (logprob) + 16 (fwd_w) + 1 (own label) + 5 (outputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--beta1", type=float, default=0.5)
    ap.add_argument("--energy_tol_ppb", type=int, default=10000)
    ap.add_argument("--entropy", action="store_true", help="also compute the per-node entropy")
    a = ap.parse_args()
    import torch
    from phylo_hmrf_amd import Block, synthetic, workloads
    from phylo_hmrf_amd.tree import PhyloTree
    blocks, S, K, nn, desc = workloads.workload(a.workload)
    rng = np.random.default_rng(a.seed)
    tree = PhyloTree(synthetic.tree_for(S))
    params = synthetic.sample_ou_params(rng, tree, K)
    means, covars = tree.mean_cov(params, 2e-3)
    dev = torch.device("cuda", 0)
    ms = dict(emission=0.0, solve=0.0, summary=0.0, d2h=0.0)
    n_all, e_all, conf_sum = 0, 0.0, 0.0
    for bi, (H, W, diag) in enumerate(blocks):
        n = workloads.block_nodes(H, W, diag)
        Xd = synthetic.device_observations(torch, dev, a.seed * 1000 + bi, H, W, diag, K, means, covars)
        torch.cuda.synchronize()
        b = Block(n, S, K)
        b.set_observations_dev(Xd.data_ptr())
        b.sync()
        b.build_grid_graph(H, W, diag, nn, a.beta1)
        b.sync()
        del Xd
        t0 = time.perf_counter()
        b.emission(means, covars)
        b.sync()
        t1 = time.perf_counter()
        b.solve_fast(a.beta, init_mode=1, energy_tol_ppb=a.energy_tol_ppb)
        t2 = time.perf_counter()
        conf, top, _ = b.posterior_summary(a.beta, 0, want_entropy=a.entropy)
        t3 = time.perf_counter()
        buf = torch.empty(n * (9 if a.entropy else 5), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        buf.cpu()
        t5 = time.perf_counter()
        del buf
        ms["emission"] += 1e3 * (t1 - t0)
        ms["solve"] += 1e3 * (t2 - t1)
        ms["summary"] += 1e3 * (t3 - t2)
        ms["d2h"] += 1e3 * (t5 - t4)
        e_all += b.energy(a.beta)[0]
        conf_sum += float(conf.astype(np.float64).sum())
        n_all += n
        b.close()
        torch.cuda.empty_cache()
    print(json.dumps(dict(workload=a.workload, desc=desc, nodes=n_all, blocks=len(blocks), K=K,
                          ms={k: round(v, 2) for k, v in ms.items()}, energy=e_all, mean_conf=conf_sum / max(n_all, 1),
                          summary_bytes_per_node=4 * K + 16 + 1 + (9 if a.entropy else 5))))


if __name__ == "__main__":
    main()
