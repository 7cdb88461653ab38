#!/usr/bin/env python3
"""Time the comparison of two state maps on a synthetic workload's label maps (default cfg3: whole genome at 50 kb, 26
blocks, 88.8 M nodes, K = 20).  Map A is tools/smooth_time.py's (synthetic.label_image with salt-and-pepper noise); map B is
A with --patches seeded rectangles per block (sides up to --side bins) relabelled.  Both maps are on the GPU before anything
is timed.  Per stage, summed over the blocks, in milliseconds by HIP events around the library call (each call allocates its
scratch, runs its kernels and reads a few words back before it returns):

    contingency       phmrf_label_contingency
    diff_components   phmrf_diff_domains with capacity 0: diff codes and bands, union-find, areas, the count of the domains
    whole_call        phmrf_diff_domains with the table (65,536 rows, asked again with the count when that is too few)
    domain_stats      whole_call - diff_components: compaction, bounding boxes, histograms, rows

with the bytes per node each stage has to move at the least (union-find traffic, which depends on the map, left out) and
the share of the 8 TB/s HBM peak that amounts to, and the host's time for the same answers on this machine:
np.bincount(a * KB + b) over all nodes, and scipy.ndimage.label (3 x 3 structure) on every block's full matrix of the
differing bin pairs.  `states` is compare_states end to end (host -> device, both passes, device -> host).  One JSON object,
printed and written to --out.
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
# the least each stage moves per node: the two maps; then the two maps again, diff written, read by the union-find's init
# (+ comp written), comp read and written by the flatten, comp read (at the differing nodes only: an upper figure) and the
# zeroed acc / mirror by the areas, comp and diff read by the count
BYTES_PER_NODE = dict(contingency=2, diff_components=2 + 1 + (1 + 4) + (4 + 4) + (4 + 9) + 5)


def relabel_patches(rng, b, row, K, patches, side):
    """relabel `patches` rectangles of the region's matrix in place, in node space (a diagonal block: the part with j >= i)"""
    H, W, diag = int(row[3]), int(row[4]), int(row[8])
    for _ in range(patches):
        i0, j0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        h, w, shift = int(rng.integers(1, side + 1)), int(rng.integers(1, side + 1)), int(rng.integers(1, K))
        for i in range(i0, min(H, i0 + h)):
            lo, hi = (max(j0, i), min(W, j0 + w)) if diag else (j0, min(W, j0 + w))
            if lo >= hi:
                continue
            first = i * W - i * (i - 1) // 2 - i if diag else i * W            # node of (i, j) = first + j
            b[first + lo:first + hi] = (b[first + lo:first + hi] + shift) % K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--patches", type=int, default=40)
    ap.add_argument("--side", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of every call; the fastest counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_time.json"))
    a = ap.parse_args()
    import torch
    from scipy import ndimage
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib, compare
    from phylo_hmrf_amd.smooth import default_max_area
    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    rng = np.random.default_rng(a.seed + 1)
    sb = sv.copy()
    for row in lv:
        relabel_patches(rng, sb[row[1]:row[2]], row, K, a.patches, a.side)
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    a_t, b_t = torch.from_numpy(sv).to(dev), torch.from_numpy(sb).to(dev)

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

    ms = dict(contingency=0.0, diff_components=0.0, whole_call=0.0)
    per_block = []
    table_total = np.zeros((K, K), dtype=np.int64)
    domains = 0
    for row in lv:
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        pa, pb = ctypes.c_void_p(a_t[lo:hi].data_ptr()), ctypes.c_void_p(b_t[lo:hi].data_ptr())
        C = np.zeros(K * K, dtype=np.int64)
        t_c, _ = timed(lambda: _lib.check(L.phmrf_label_contingency(pa, pb, hi - lo, K, K, _lib.ptr_i64(C), st)))
        table_total += C.reshape(K, K)
        area = default_max_area(H) + 1

        def diff(capacity):
            table = np.zeros((max(capacity, 1), compare.DOMAIN_COLS), dtype=np.int64)
            found = ctypes.c_int64(0)
            _lib.check(L.phmrf_diff_domains(pa, pb, None, None, None, H, W, diag, int(row[6]) - int(row[5]), K, K, 0.0, area,
                                            None, capacity, _lib.ptr_i64(table), ctypes.byref(found), None, st))
            return int(found.value)

        t_d, found = timed(lambda: diff(0))
        t_w, _ = timed(lambda: diff(max(found, 1) if found > compare.FIRST_CAPACITY else compare.FIRST_CAPACITY))
        ms["contingency"] += t_c
        ms["diff_components"] += t_d
        ms["whole_call"] += t_w
        domains += found
        per_block.append(dict(H=H, W=W, diagonal=diag, nodes=hi - lo, domains=found, contingency_ms=round(t_c, 4),
                              diff_components_ms=round(t_d, 4), whole_call_ms=round(t_w, 4)))
    ms["domain_stats"] = ms["whole_call"] - ms["diff_components"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = compare.compare_states(sv, sb, lv)
    ms["states"] = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(res["contingency"], table_total) and res["domains"].shape[0] == domains

    host = {}
    t0 = time.perf_counter()
    ref = np.bincount(sv.astype(np.int64) * K + sb, minlength=K * K).reshape(K, K)
    host["bincount"] = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(ref, table_total)
    t0 = time.perf_counter()
    components = 0
    for row in lv:
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        differs = sv[lo:hi] != sb[lo:hi]
        if diag:
            M = np.zeros((H, H), dtype=bool)
            iu = np.triu_indices(H)
            M[iu] = differs
            M |= M.T
        else:
            M = differs.reshape(H, W)
        components += ndimage.label(M, structure=np.ones((3, 3), dtype=bool))[1]
    host["label"] = 1e3 * (time.perf_counter() - t0)

    n = int(sv.size)
    share = {k: BYTES_PER_NODE[k] * n / (ms[k] * 1e-3) / HBM_PEAK for k in BYTES_PER_NODE}
    out = dict(workload=a.workload, desc=desc, nodes=n, blocks=int(lv.shape[0]), K=K, noise=a.noise, patches=a.patches,
               side=a.side, repeats=a.repeats, differing_nodes=int((sv != sb).sum()), domains=domains,
               host_components_all_areas=components, agreement=res["agreement"], ari=res["ari"], nmi=res["nmi"],
               ms={k: round(v, 3) for k, v in ms.items()}, bytes_per_node=BYTES_PER_NODE,
               hbm_share={k: round(v, 4) for k, v in share.items()}, host_ms={k: round(v, 1) for k, v in host.items()},
               host_threads=min(16, os.cpu_count() or 1), per_block=per_block)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
