#!/usr/bin/env python3
"""Time the raw loader's three smoothing filters, host against GPU, on seeded synthetic contact-map planes: log1p of
uniform noise plus a distance-decay ridge along the diagonal, non-negative, symmetric.  The planes are square, at the sides
given by --sizes (default 652, the chr22 block of BASELINE config 1, and 4979, the chr1 plane of the 50 kb workload) or at the
distinct sides of the diagonal blocks of --workload (a name of phylo_hmrf_amd/workloads.py).

One JSON line per filter and size, times in seconds:

    host        the host function as the loader calls it (one run; skipped above --skip-host-above pixels per side:
                the bilateral filter takes about a minute at 4979)
    device      the `*_device` function end to end: upload of the plane, the call, download of the result
                (one warm-up call, then the median of --repeat)
    kernel      HIP events around the library call alone, the plane already in device memory (one warm-up call, then the
                median of --repeat).  For the bilateral filter the call holds the min / max reduction, the upload of the two
                tables and the filter kernel; for the Gaussian the upload of the weights and the two passes
    diffusion   hbm_fraction = 8 B per pixel and iteration over the kernel time, as a share of the 8 TB/s HBM peak
    bilateral   taps_per_s = pixels x window^2 over the kernel time

The colour table's placement (LDS or global memory) is a build-time choice of csrc/preprocess.hip: time the other one by
loading a library built with -DPHMRF_BILATERAL_LUT_GLOBAL through PHMRF_LIB (tools/variant.sh).  The kernels' own times
come from a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/preprocess_time.py --skip-host-above 0.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8e12                # bytes / s


def plane(side, seed):
    """float64 [side, side]: symmetric, non-negative, log1p(uniform noise + a ridge that decays with |i - j|)"""
    rng = np.random.default_rng(seed)
    a = rng.random((side, side)) * 4.0
    a = np.triu(a) + np.triu(a, 1).T
    d = np.abs(np.arange(side)[:, None] - np.arange(side)[None, :])
    return np.log1p(a + 60.0 / (1.0 + d))


def timed(fn, repeat):
    """-> median seconds of `repeat` runs of fn after one warm-up run (fn ends in a device synchronise or a copy back)"""
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def event_timed(torch, fn, repeat):
    """-> median seconds between two HIP events around fn, after one warm-up run"""
    fn()
    ts = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="652,4979", help="sides of the square planes")
    ap.add_argument("--workload", default="", help="take the sides of this workload's diagonal blocks instead")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-host-above", type=int, default=1 << 30, help="no host run above this many pixels per side")
    ap.add_argument("--filters", default="diffusion,bilateral,gaussian")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    import scipy.ndimage
    from phylo_hmrf_amd import _lib, preprocess, workloads
    if a.workload:
        sizes = sorted(set(H for H, W, diag in workloads.workload(a.workload)[0] if diag))
    else:
        sizes = [int(s) for s in a.sizes.split(",")]
    L = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    niter, kappa, gamma = 5, 50.0, 0.1                      # the loader's filter_mode 0
    sc, ss, bins = 0.5, 5.0, 10000                          # the loader's filter_mode 1: window 31
    win = max(5, 2 * int(np.ceil(3 * ss)) + 1)
    sigma = 0.25                                            # the CLI's default --filter_sigma
    lines = []
    for side in sizes:
        img = plane(side, a.seed)
        px = side * side
        host_ok = side <= a.skip_host_above
        for name in a.filters.split(","):
            r = dict(filter=name, side=side, pixels=px, library=os.path.basename(_lib.LIB_PATH))
            if name == "diffusion":
                host = lambda: preprocess.anisotropic_diffusion(img, niter=niter, kappa=kappa, gamma=gamma, option=1)
                device = lambda: preprocess.anisotropic_diffusion_device(img, niter=niter, kappa=kappa, gamma=gamma, option=1)
                d_img = torch.from_numpy(img.astype(np.float32)).to(dev)
                d_tmp = torch.empty_like(d_img)
                call = lambda: _lib.check(L.phmrf_filter_diffusion(vp(d_img), vp(d_tmp), side, side, niter, kappa, gamma, 1, st))
                r.update(niter=niter, kappa=kappa)
            elif name == "bilateral":
                host = lambda: preprocess.denoise_bilateral(img, sigma_color=sc, sigma_spatial=ss)
                device = lambda: preprocess.denoise_bilateral_device(img, sigma_color=sc, sigma_spatial=ss)
                d_img = torch.from_numpy(img).to(dev)
                d_out = torch.empty_like(d_img)
                call = lambda: _lib.check(L.phmrf_filter_bilateral(vp(d_img), vp(d_out), side, side, sc, ss, 0, bins, st))
                r.update(sigma_color=sc, sigma_spatial=ss, window=win, bins=bins)
            elif name == "gaussian":
                host = lambda: scipy.ndimage.gaussian_filter(img, sigma)
                device = lambda: preprocess.gaussian_filter_device(img, sigma)
                d_img = torch.from_numpy(img).to(dev)
                d_out, d_tmp = torch.empty_like(d_img), torch.empty_like(d_img)
                call = lambda: _lib.check(L.phmrf_filter_gaussian(vp(d_img), vp(d_out), vp(d_tmp), side, side, sigma, 4.0, st))
                r.update(sigma=sigma)
            else:
                raise SystemExit("unknown filter %r" % name)
            if host_ok:
                t0 = time.perf_counter()
                host()
                r["host_s"] = time.perf_counter() - t0
            else:
                r["host_s"] = None
            r["device_s"] = timed(device, a.repeat)
            r["kernel_s"] = event_timed(torch, call, a.repeat)
            r["copies_s"] = r["device_s"] - r["kernel_s"]
            if r["host_s"] is not None:
                r["host_over_device"] = r["host_s"] / r["device_s"]
            if name == "diffusion":
                r["bytes_per_s"] = 8.0 * px * niter / r["kernel_s"]
                r["hbm_fraction"] = r["bytes_per_s"] / HBM_PEAK
            if name == "bilateral":
                r["taps_per_s"] = float(px) * win * win / r["kernel_s"]
            line = json.dumps({k: (round(v, 6) if isinstance(v, float) and abs(v) < 1e6 else v) for k, v in r.items()})
            print(line, flush=True)
            lines.append(line)
            del d_img
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
