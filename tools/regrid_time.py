#!/usr/bin/env python3
"""Time the resampling of a state map onto another grid (phmrf_regrid_states) on three inputs, K = 20:

    chr1_10k_50k   one diagonal block of chr1's size at 10 kb (24,800 bins, 307.5 M stored bin pairs) onto its 50 kb grid
                   (a = 1, b = 5: 4,960 bins, 12.3 M target cells): the lane kernel.  The block is a 50 kb label image refined
                   five times with --noise of its 10 kb bin pairs redrawn, so most target cells are mixed
    genome_split   the 26 blocks of tools/smooth_time.py's genome map (cfg3: whole genome at 50 kb, 88.8 M nodes) onto a grid
                   with another split at a = b = 1: a chromosome held as one block is cut into two arms and the block between
                   them at its middle, chr3 and chr6 -- held as three blocks -- become one: 62 target regions, one call each
    large_ratio    the first block read as 5 kb bins onto 1 Mb (a = 1, b = 200: 124 bins, 7,750 target cells of 200 x 200
                   source cells): the wave kernel

The map is on the GPU before anything is timed.  Per input, summed over its calls, in milliseconds by HIP events around the
library call (each call makes its axis and piece tables, allocates, runs its kernel, copies the planes into the caller's device
buffers and the counts to the host before it returns), the fastest of --repeats.  Beside it:
    host_ms    the restatement of tests/regrid_reference.py on this machine's CPU, on a SUBSET -- a window of --window source
               bins on the diagonal of the first chromosome, cut out as a map of its own, onto the same kind of grid -- and scaled
               by target cells / the subset's target cells.  The device regrids the same window in a call of its own and the planes
               and counts of the two must be equal.
    render_ms  chr1_10k_50k only: phmrf_render_states at factor 5 on the same block with its copy of the three pixel planes to
               the host, a yardstick for the same traffic; its state plane must equal the regridded map at min_cover = 1.
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
NOT_MEASURED = ["the kernels' own time apart from the call's fixed cost (no kernel trace was taken): the host's axis and piece tables, "
                "allocation, the uploads, the device-to-device copies of the planes and the waits are inside every figure",
                "the threshold between the lane-per-cell and the wave-per-cell kernel (SMALL_AREA = 256; no other value was run)",
                "the tile (LANES = 128), the waves of a workgroup and the grid caps",
                "rational ratios, refining, other K than 20, maps with less or more noise",
                "regrid_states / regrid_files end to end (host -> device, the planes back, conf and cover, the .mat and the text)",
                "bytes moved and the share of the HBM peak", "the spread between runs (the fastest of --repeats counts)"]


def layout(regions):
    """(H, W, start_bin1, start_bin2, diagonal, chrom) -> len_vec, the nodes back to back"""
    rows, at = [], 0
    for r, (H, W, s1, s2, diag, chrom) in enumerate(regions):
        n = H * (H + 1) // 2 if diag else H * W
        rows.append([n, at, at + n, H, W, s1, s2, r, diag, chrom])
        at += n
    return np.array(rows, dtype=np.int64)


def other_split(lv):
    """the target regions of genome_split: per chromosome of one block two arms and the block between them, cut at the middle;
    per chromosome of several blocks one diagonal block over all its bins"""
    regions = []
    for c in np.unique(lv[:, 9]):
        rows = lv[lv[:, 9] == c]
        bins = max(max(int(r[5] + r[3]), int(r[6] + r[4])) for r in rows)
        if rows.shape[0] == 1:
            h = bins // 2
            regions += [(h, h, 0, 0, 1, int(c)), (bins - h, bins - h, h, h, 1, int(c)), (h, bins - h, 0, h, 0, int(c))]
        else:
            regions.append((bins, bins, 0, 0, 1, int(c)))
    return layout(regions)


def window_of_block(sv, row, n):
    """the first n bins of a diagonal block as a map of its own -> its state_vec (one diagonal block of n bins)"""
    lo, H = int(row[1]), int(row[3])
    first = lambda i: lo + i * H - (i * (i - 1)) // 2
    return np.concatenate([sv[first(i):first(i) + n - i] for i in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--bins", type=int, default=24800, help="chr1_10k_50k and large_ratio: the block's side in source bins")
    ap.add_argument("--window", type=int, default=300, help="source bins of the subset the host restates (a multiple of 5)")
    ap.add_argument("--repeats", type=int, default=3, help="timed repetitions of every call; the fastest counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regrid_time.json"))
    a = ap.parse_args()
    import torch
    from smooth_time import genome_maps
    from phylo_hmrf_amd import _lib, regrid, synthetic
    from phylo_hmrf_amd.render import default_palette
    from tests import regrid_reference
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    K = 20

    def call(m_t, n, regs, row, aa, bb, min_cover, out):
        """one target region (a len_vec row) into the planes `out` = (state, support, covered) at the row's slice"""
        lo, H, W, t1, t2, diag = (int(row[x]) for x in (1, 3, 4, 5, 6, 8))
        hist, mixed = np.zeros(K + 1, dtype=np.int64), ctypes.c_int64(0)
        _lib.check(L.phmrf_regrid_states(ctypes.c_void_p(m_t.data_ptr()), n, regs.shape[0], _lib.ptr_i64(regs), K, aa, bb, H, W, diag,
                                         t1, t2, min_cover, K, ctypes.c_void_p(out[0].data_ptr() + lo),
                                         ctypes.c_void_p(out[1].data_ptr() + 4 * lo), ctypes.c_void_p(out[2].data_ptr() + 4 * lo),
                                         _lib.ptr_i64(hist), ctypes.byref(mixed), st))
        return hist, int(mixed.value)

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

    def planes_for(D):
        n = int(D[:, 2].max())
        return (torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev))

    def run(name, m_t, n, lv, D, aa, bb, min_cover, window_sv, window_D):
        """the calls of the target len_vec D, timed; the subset `window_sv` (one diagonal block) onto window_D on both sides"""
        out = planes_for(D)
        ms, hist, mixed = 0.0, np.zeros(K + 1, dtype=np.int64), 0
        for row in D:
            regs = np.ascontiguousarray(lv[lv[:, 9] == row[9]][:, [1, 3, 4, 5, 6, 8]], dtype=np.int64)
            t, (h, m) = timed(lambda: call(m_t, n, regs, row, aa, bb, min_cover, out))
            ms, hist, mixed = ms + t, hist + h, mixed + m
        cells = int(hist.sum())
        # the subset on the device and on the host
        w = int(round((np.sqrt(8 * window_sv.size + 1) - 1) / 2))
        w_lv = layout([(w, w, 0, 0, 1, 1)])
        w_t = torch.from_numpy(window_sv).to(dev)
        w_out = planes_for(window_D)
        w_regs = np.ascontiguousarray(w_lv[:, [1, 3, 4, 5, 6, 8]], dtype=np.int64)
        got = [call(w_t, window_sv.size, w_regs, row, aa, bb, min_cover, w_out) for row in window_D]
        t0 = time.perf_counter()
        want = regrid_reference.regrid(window_sv, w_lv, window_D, aa, bb, K, min_cover)
        host_ms = 1e3 * (time.perf_counter() - t0)
        agree = bool(np.array_equal(w_out[0].cpu().numpy(), want["state_vec"]) and
                     np.array_equal(w_out[1].cpu().numpy().view(np.uint32), want["support"]) and
                     np.array_equal(w_out[2].cpu().numpy().view(np.uint32), want["covered"]) and
                     np.array_equal(np.array([g[0] for g in got]), want["hist_region"]) and
                     np.array_equal(np.array([g[1] for g in got]), want["mixed_region"]))
        sub_cells = int(window_D[:, 0].sum())
        res = dict(a=aa, b=bb, lane_kernel=bool(regrid.is_small(aa, bb)), source_nodes=int(n), source_regions=int(lv.shape[0]),
                   calls=int(D.shape[0]), target_cells=cells, called=int(cells - hist[K]), mixed=mixed, min_cover=int(min_cover),
                   ms=round(ms, 3), subset_source_bins=w, subset_cells=sub_cells, subset_host_ms=round(host_ms, 1),
                   host_ms_scaled=round(host_ms * cells / sub_cells, 1), planes_agree=agree,
                   host_over_device=round(host_ms * cells / sub_cells / ms, 1))
        print("%s: %s" % (name, json.dumps(res)), flush=True)
        assert agree, "%s: the subset's planes differ" % name
        return res, out

    out = dict(repeats=a.repeats, K=K, noise=a.noise, inputs={})
    # ---- one block of chr1's size: a 50 kb label image refined five times, with noise, made on the GPU
    B, f = a.bins, 5
    rng = np.random.default_rng(a.seed)
    coarse = synthetic.label_image(rng, B // f, B // f, K).astype(np.uint8)
    torch.manual_seed(a.seed)
    M = torch.from_numpy(coarse).to(dev).repeat_interleave(f, 0).repeat_interleave(f, 1)
    hit = torch.rand((B, B), device=dev) < a.noise
    M = torch.where(hit, torch.randint(0, K, (B, B), device=dev, dtype=torch.uint8), M)
    del hit
    iu = torch.triu_indices(B, B, device=dev)
    m_t = M[iu[0], iu[1]].contiguous()
    del iu, M
    n = int(m_t.numel())
    lv = layout([(B, B, 0, 0, 1, 1)])
    sv_window = window_of_block(m_t[:a.window * B].cpu().numpy(), lv[0], a.window)
    print("block ready: %d bins, %d nodes" % (B, n), flush=True)
    warm = planes_for(layout([(8, 8, 0, 0, 1, 1)]))
    call(m_t, n, lv[:, [1, 3, 4, 5, 6, 8]].copy(), layout([(8, 8, 0, 0, 1, 1)])[0], 1, 5, 1, warm)     # (code objects loaded before the first timing)
    call(m_t, n, lv[:, [1, 3, 4, 5, 6, 8]].copy(), layout([(2, 2, 0, 0, 1, 1)])[0], 1, 200, 1, warm)
    D = regrid.derive_len_vec(lv, 10000, 50000)
    res, planes = run("chr1_10k_50k", m_t, n, lv, D, 1, 5, 1, sv_window, layout([(a.window // 5, a.window // 5, 0, 0, 1, 1)]))
    # the yardstick: the same block through phmrf_render_states at factor 5
    h = -(-B // f)
    px = np.zeros((3, h, h), dtype=np.uint8)
    palette, extra = np.ascontiguousarray(default_palette(K), dtype=np.uint8), np.zeros(6, dtype=np.uint8)
    render_ms, _ = timed(lambda: _lib.check(L.phmrf_render_states(
        ctypes.c_void_p(m_t.data_ptr()), None, None, B, B, 1, K, f, palette.ctypes.data_as(ctypes.c_void_p),
        extra.ctypes.data_as(ctypes.c_void_p), 0, px.ctypes.data_as(ctypes.c_void_p), None, st)))
    same = bool(np.array_equal(px[0][np.triu_indices(h)], planes[0].cpu().numpy()))
    res.update(render_ms=round(render_ms, 3), render_over_regrid=round(render_ms / res["ms"], 2), render_state_plane_equal=same)
    print("render at factor 5: %.3f ms, state plane equal: %s" % (render_ms, same), flush=True)
    assert same, "the render vote and the regridded map differ"
    out["inputs"]["chr1_10k_50k"] = res
    del planes
    # ---- the same block read as 5 kb bins onto 1 Mb
    D = regrid.derive_len_vec(lv, 5000, 1000000)
    w3 = 2 * 200
    sv_window3 = sv_window if a.window >= w3 else window_of_block(m_t[:w3 * B].cpu().numpy(), lv[0], w3)
    out["inputs"]["large_ratio"], _ = run("large_ratio", m_t, n, lv, D, 1, 200, 20000, sv_window3, layout([(2, 2, 0, 0, 1, 1)]))
    del m_t
    # ---- the genome at 50 kb onto another split
    sv, lv, K2, desc = genome_maps(a.workload, a.seed, a.noise)
    assert K2 == K
    print("genome maps ready: %d nodes" % sv.size, flush=True)
    m_t = torch.from_numpy(sv).to(dev)
    first = lv[lv[:, 9] == lv[0, 9]]
    assert first.shape[0] == 1 and first[0, 8] == 1 and first[0, 3] >= a.window
    half = a.window // 2
    window_D = layout([(half, half, 0, 0, 1, 1), (a.window - half, a.window - half, half, half, 1, 1), (half, a.window - half, 0, half, 0, 1)])
    res, _ = run("genome_split", m_t, sv.size, lv, other_split(lv), 1, 1, 1, window_of_block(sv, first[0], a.window), window_D)
    out["inputs"]["genome_split"] = dict(res, workload=a.workload, desc=desc)
    out["not_measured"] = NOT_MEASURED
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
