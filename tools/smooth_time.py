#!/usr/bin/env python3
"""Time the post-processing on a synthetic workload's label maps (default cfg3: whole genome at 50 kb, 26 blocks, 88.8 M
nodes, K = 20): every block's map is synthetic.label_image with salt-and-pepper noise (a share --noise of the bins takes a
uniformly drawn state).  Printed as one JSON line, in milliseconds:

    device     phmrf_smooth_labels over all blocks, labels already on the GPU (each call synchronises: it reads back the
               number of small components to size the vote histograms)
    states     smooth_states end to end (host -> device, the pass, device -> host)
    write_ori, write_smooth   write_state_files of the input and of the smoothed states (--out, removed afterwards)

The kernels' own times come from a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/smooth_time.py --no-write
(smooth_*_kernel, the components_* kernels of csrc/components.h and the cc_*_grid / cc_flatten kernels of the union-find).
"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def genome_maps(workload, seed, noise):
    """-> (state_vec uint8, len_vec, K, description) of the workload's blocks, in workloads.genome_blocks' order: one diagonal
    block per chromosome, for chr3 and chr6 the two arms' diagonal blocks and the off-diagonal block between them"""
    from phylo_hmrf_amd import synthetic, workloads
    blocks, S, K, nn, desc = workloads.workload(workload)
    chroms = []
    for c in range(1, 23):
        chroms += [c] * (3 if c in workloads.SPLIT else 1)
    if len(chroms) != len(blocks):
        chroms = list(range(1, len(blocks) + 1))                # (a single-block workload: one chromosome per block)
    rng = np.random.default_rng(seed)
    parts, rows, start = [], [], 0
    for bi, (H, W, diag) in enumerate(blocks):
        img = synthetic.label_image(rng, H, W, K)
        hit = rng.random((H, W)) < noise
        img[hit] = rng.integers(0, K, int(hit.sum()))
        lab = img[np.triu_indices(H)] if diag else img.reshape(-1)
        n = lab.shape[0]
        parts.append(lab.astype(np.uint8))
        first = bi > 0 and chroms[bi - 1] == chroms[bi]          # the second arm (or the off-diagonal block) of a split
        s2 = blocks[bi - 1][0] + 70 if first else 0               # (bins past the first arm, beyond the centromere gap)
        rows.append([n, start, start + n, H, W, s2 if first and diag else 0, s2 if first else 0, bi, 1 if diag else 0,
                     chroms[bi]])
        start += n
    return np.concatenate(parts), np.array(rows, dtype=np.int64), K, desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--iter", type=int, default=1)
    ap.add_argument("--out", default="", help="directory for the written files (default: a temporary one)")
    ap.add_argument("--no-write", action="store_true", help="time the device pass only")
    a = ap.parse_args()
    import torch
    from phylo_hmrf_amd import _lib
    from phylo_hmrf_amd.smooth import default_max_area, smooth_states, write_state_files
    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    ms = dict(device=0.0)
    counts = np.zeros(3, dtype=np.int64)
    for row in lv:
        src = torch.from_numpy(sv[row[1]:row[2]]).to(dev)
        dst = torch.empty_like(src)
        c = np.zeros(3 * a.iter, dtype=np.int64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(L.phmrf_smooth_labels(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), int(row[3]),
                                         int(row[4]), int(row[8]), K, a.window, default_max_area(row[3]), a.iter,
                                         _lib.ptr_i64(c), ctypes.c_void_p(st)))
        ms["device"] += 1e3 * (time.perf_counter() - t0)
        counts += c.reshape(a.iter, 3).sum(axis=0)
        del src, dst
    t0 = time.perf_counter()
    smooth, _ = smooth_states(sv, lv, window=a.window, n_iter=a.iter)
    ms["states"] = 1e3 * (time.perf_counter() - t0)
    sizes = {}
    if not a.no_write:
        out = a.out or tempfile.mkdtemp(prefix="smooth_time_")
        try:
            for annot, states in (("ori", sv), ("smooth", smooth)):
                t0 = time.perf_counter()
                files = write_state_files(states, lv, 50000, out, annot)
                ms["write_" + annot] = 1e3 * (time.perf_counter() - t0)
                sizes[annot] = sum(os.path.getsize(f) for f in files)
        finally:
            if not a.out:
                shutil.rmtree(out, ignore_errors=True)
    print(json.dumps(dict(workload=a.workload, desc=desc, nodes=int(sv.size), blocks=int(lv.shape[0]), K=K, noise=a.noise,
                          window=a.window, iter=a.iter, ms={k: round(v, 2) for k, v in ms.items()},
                          small_components=int(counts[0]), relabelled=int(counts[1]), nodes_changed=int(counts[2]),
                          changed_vs_states=int((smooth != sv).sum()), bytes_written=sizes)))


if __name__ == "__main__":
    main()
