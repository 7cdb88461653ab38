#!/usr/bin/env python3
"""Time the domains and the state adjacency of one state map on a synthetic workload's label maps (default cfg3: whole genome
at 50 kb, 26 blocks, 88.8 M nodes, K = 20), for two maps of the same blocks:

    noisy      tools/compare_time.py's map A (synthetic.label_image with salt-and-pepper noise)
    dominant   the noisy map with state 0 written over about --share of every block: a second, coarser label image (mean
               run 100 bins) picks the regions that keep their states.  Same node count, one state in components of millions
               of nodes: what the carried roots of the area and statistics passes are for.

Both maps are on the GPU before anything is timed.  Per call, summed over the blocks, in milliseconds by HIP events around the
library call (each call allocates its scratch, runs its kernels and reads a few words back before it returns), the fastest
of --repeats:

    adjacency   phmrf_state_adjacency
    domains     phmrf_state_domains with the node ids and a table of 65,536 rows (asked again with the count when that is
                too few), the default area rule

and the host's time on this machine for the same answers: scipy.ndimage.label (3 x 3 structure) per state on every block's
full matrix, and np.bincount over the stored edges of the four forward directions.  `dominant_over_noisy` is the ratio of
the two maps' domain calls: above 2 the large components' atomics pile up on one address.

The kernels' own time is not in this run: a kernel trace slows the host.  Take it in a run of its own,
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/domains_time.py --kernel-pass noisy
(one domain call per block and nothing else), and fold the two *kernel_stats.csv into the JSON with
    python tools/domains_time.py --fold noisy=FILE,dominant=FILE
which adds kernels (per kernel, summed over the blocks), kernel_ms and outside_kernels (the share of the call that is
allocation, launches, copies and waits).
One JSON object, printed and written to --out.
"""
import argparse
import csv
import ctypes
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
KERNELS = ("domains_", "components_", "cc_", "__amd_rocclr")   # the call's kernels in a trace: its own, csrc/components.h's, the union-find, the memsets
NOT_MEASURED = ["the adjacency kernel's own time (the kernel pass makes domain calls only)", "bytes moved and the share of the HBM peak",
                "state_domains end to end (host -> device, the calls, device -> host)", "maps with confidences",
                "other shares than --share, other K than the workload's", "the spread between runs (the fastest of --repeats counts)"]


def dominant_map(sv, lv, K, seed, share):
    """the map with state 0 over the regions a coarse label image does not pick: about `share` of every block"""
    from phylo_hmrf_amd import synthetic
    rng = np.random.default_rng(seed)
    out = sv.copy()
    for row in lv:
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        img = synthetic.label_image(rng, H, W, K, mean_run=100)
        mask = img[np.triu_indices(H)] if diag else img.reshape(-1)
        counts = np.bincount(mask, minlength=K)
        order = np.argsort(counts, kind="stable")
        cum = np.cumsum(counts[order]) / float(hi - lo)
        keep = order[:int(np.argmin(np.abs(cum - (1.0 - share)))) + 1]
        part = out[lo:hi]
        part[~np.isin(mask, keep)] = 0
    return out


def full_matrix(states, H, W, diag):
    if not diag:
        return states.reshape(H, W)
    M = np.zeros((H, H), dtype=states.dtype)
    iu = np.triu_indices(H)
    M[iu] = states
    M.T[iu] = states
    return M


def host_answers(sv, lv, K):
    """-> (ms of the labelling, ms of the adjacency, components counted on the full matrices, adjacency [K, K])"""
    from scipy import ndimage
    t_label = t_adj = 0.0
    components = 0
    adj = np.zeros((K, K), dtype=np.int64)
    structure = np.ones((3, 3), dtype=bool)
    for row in lv:
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        M = full_matrix(sv[lo:hi], H, W, diag)
        t0 = time.perf_counter()
        for k in np.unique(M):
            components += ndimage.label(M == k, structure=structure)[1]
        t_label += time.perf_counter() - t0
        t0 = time.perf_counter()
        A = M.astype(np.int32) * K
        ii, jj = np.indices((H, W), sparse=True)
        raw = np.zeros(K * K, dtype=np.int64)
        for di, dj in ((0, 1), (1, -1), (1, 0), (1, 1)):            # E, SW, S, SE of the first node
            a = A[0:H - di, max(0, -dj):W - max(0, dj)]
            b = M[di:H, max(0, dj):W + min(0, dj)]
            if diag:                                                 # both ends stored: i <= j and i2 <= j2
                i, j = ii[0:H - di], jj[:, max(0, -dj):W - max(0, dj)]
                ok = (i <= j) & (i + di <= j + dj)
                raw += np.bincount((a + b)[ok], minlength=K * K)
            else:
                raw += np.bincount((a + b).reshape(-1), minlength=K * K)
        raw = raw.reshape(K, K)
        adj += raw + raw.T - np.diag(np.diagonal(raw))
        t_adj += time.perf_counter() - t0
    return 1e3 * t_label, 1e3 * t_adj, components, adj


def fold(out_path, spec):
    res = json.loads(open(out_path).read())
    for item in spec.split(","):
        name, path = item.split("=", 1)
        rows = [r for r in csv.DictReader(open(path)) if any(k in r["Name"] for k in KERNELS)]
        kernel_ms = sum(float(r["TotalDurationNs"]) for r in rows) / 1e6
        res["maps"][name]["kernel_ms"] = round(kernel_ms, 3)
        res["maps"][name]["outside_kernels"] = round(1.0 - kernel_ms / res["maps"][name]["ms"]["domains"], 4)
        short = lambda full: (re.findall(r"(\w+)\(", full) or [full])[0]
        res["maps"][name]["kernels"] = {short(r["Name"]): round(float(r["TotalDurationNs"]) / 1e6, 3) for r in rows}
    res["not_measured"] = NOT_MEASURED
    print(json.dumps(res))
    with open(out_path, "w") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--share", type=float, default=0.9, help="the dominant map: the share of a block that state 0 takes")
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of every call; the fastest counts")
    ap.add_argument("--kernel-pass", default="", help="noisy or dominant: one domain call per block and nothing else")
    ap.add_argument("--fold", default="", help="noisy=FILE,dominant=FILE: the kernel_stats.csv of the two kernel passes")
    ap.add_argument("--host-only", action="store_true", help="the host's times alone (no GPU needed; nothing is written)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "domains_time.json"))
    a = ap.parse_args()
    if a.fold:
        return fold(a.out, a.fold)
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib, domains
    from phylo_hmrf_amd.smooth import default_max_area
    sv, lv, K, desc = genome_maps(a.workload, a.seed, a.noise)
    maps = dict(noisy=sv, dominant=dominant_map(sv, lv, K, a.seed + 2, a.share))
    if a.host_only:
        for name, m in maps.items():
            t_label, t_adj, components, _ = host_answers(m, lv, K)
            print(json.dumps(dict(map=name, host_ms=dict(label=round(t_label, 1), adjacency=round(t_adj, 1)),
                                  components=components, share_of_state_0=round(float((m == 0).mean()), 4))))
        return
    import torch
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def domains_call(m_t, ids_t, row, capacity):
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        table = np.zeros((max(capacity, 1), domains.STATE_DOMAIN_COLS), dtype=np.int64)
        found, comps = ctypes.c_int64(0), np.zeros(K, dtype=np.int64)
        _lib.check(L.phmrf_state_domains(ctypes.c_void_p(m_t[lo:hi].data_ptr()), None, H, W, diag, int(row[6]) - int(row[5]), K,
                                         default_max_area(H) + 1, ctypes.c_void_p(ids_t[lo:hi].data_ptr()), capacity,
                                         _lib.ptr_i64(table), ctypes.byref(found), _lib.ptr_i64(comps), st))
        return int(found.value), table, comps

    if a.kernel_pass:
        m_t = torch.from_numpy(maps[a.kernel_pass]).to(dev)
        ids_t = torch.empty(m_t.numel(), dtype=torch.int32, device=dev)
        for row in lv:
            found, _, _ = domains_call(m_t, ids_t, row, domains.FIRST_CAPACITY)
            assert found <= domains.FIRST_CAPACITY
        torch.cuda.synchronize()
        return

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

    res = {}
    for name, m in maps.items():
        m_t = torch.from_numpy(m).to(dev)
        ids_t = torch.empty(m_t.numel(), dtype=torch.int32, device=dev)
        domains_call(m_t, ids_t, lv[-1], domains.FIRST_CAPACITY)              # (code objects loaded before the first timing)
        ms = dict(adjacency=0.0, domains=0.0)
        adj_total = np.zeros((K, K), dtype=np.int64)
        comps_total, listed, largest, per_block = 0, 0, 0, []
        for row in lv:
            lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
            adj = np.zeros(K * K, dtype=np.int64)
            t_a, _ = timed(lambda: _lib.check(L.phmrf_state_adjacency(ctypes.c_void_p(m_t[lo:hi].data_ptr()), H, W, diag, K,
                                                                      _lib.ptr_i64(adj), st)))
            found, _, _ = domains_call(m_t, ids_t, row, 0)
            t_d, (found, table, comps) = timed(lambda: domains_call(m_t, ids_t, row, max(found, domains.FIRST_CAPACITY)))
            ms["adjacency"] += t_a
            ms["domains"] += t_d
            adj_total += adj.reshape(K, K)
            comps_total += int(comps.sum())
            listed += found
            largest = max(largest, int(table[:found, 5].max()) if found else 0)
            per_block.append(dict(H=H, W=W, diagonal=diag, nodes=hi - lo, domains=found, components=int(comps.sum()),
                                  adjacency_ms=round(t_a, 4), domains_ms=round(t_d, 4)))
        del m_t, ids_t
        t_label, t_adj, components_full, adj_host = host_answers(m, lv, K)
        assert np.array_equal(adj_host, adj_total)
        res[name] = dict(share_of_state_0=round(float((m == 0).mean()), 4), largest_domain_nodes=largest, domains=listed,
                         components=comps_total, host_components_full_matrix=components_full,
                         discordant_edges=int(np.triu(adj_total, 1).sum()), ms={k: round(v, 3) for k, v in ms.items()},
                         host_ms=dict(label=round(t_label, 1), adjacency=round(t_adj, 1)), per_block=per_block)
    out = dict(workload=a.workload, desc=desc, nodes=int(sv.size), blocks=int(lv.shape[0]), K=K, noise=a.noise, share=a.share,
               repeats=a.repeats, host_threads=min(16, os.cpu_count() or 1), maps=res,
               dominant_over_noisy=round(res["dominant"]["ms"]["domains"] / res["noisy"]["ms"]["domains"], 3),
               not_measured=NOT_MEASURED + ["the kernels' own time (--kernel-pass, --fold)"])
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
