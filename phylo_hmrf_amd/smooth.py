"""Post-processing of a state map (the reference's processing/*.m, outputfile_description.txt "Post-processing"): the
small-region smoothing on the GPU and the export of the states in genome coordinates.

`smooth_states(state_vec, len_vec, window=5, max_area=None, n_iter=1)` runs, region by region, the reference's smoothing
(small_region_test.m with query_neighbor_state_test.m) through phmrf_smooth_labels (csrc/smooth.hip): every 8-connected
same-state component of the region's full matrix with area <= max_area takes the state that holds more than half of the
other states in the window x window neighbourhoods of its pixels.  max_area=None is read_state_test.m's rule: 80, or 25 for
a region less than 100 bins high.

`write_state_files(state_vec, len_vec, resolution, output_path, annotation)` writes, per chromosome of len_vec column 10,
what write_stateToFile_test.m writes: estimate_test<chrom>.<annotation>.txt (one line per bin pair: chrom, start1, stop1,
chrom, start2, stop2, state + 1, tab separated, CRLF line ends) and test<chrom>.region.txt (the regions' columns 1 - 7 with
1-based start / stop indices counted within the chromosome).  Each node is written beside its own bin pair (the script
pairs a diagonal block's row-major states with column-major bin pairs).  Host only: the lines are
assembled from per-bin and per-state byte strings with NumPy, never formatted line by line.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

from .maps import MAX_STATES, check_len_vec, check_state_vec, default_max_area, device, regions, stem

RATIO = 0.5                  # read_state_test.m's call of query_neighbor_state_test (fixed in the kernel: 2 count > total)


def smooth_states(state_vec, len_vec, window=5, max_area=None, n_iter=1):
    """-> (smoothed state_vec, same dtype and shape; counts int64 [regions, n_iter, 3]: per pass the small components, the
    components relabelled and the nodes changed, as stored -- a diagonal block's mirror twins count once).  Nodes outside
    every region of len_vec keep their states."""
    states = check_state_vec(state_vec)
    L = check_len_vec(len_vec, states.shape[0])
    window, n_iter = int(window), int(n_iter)
    if window < 1:
        raise ValueError("window must be >= 1")
    if n_iter < 0:
        raise ValueError("n_iter must be >= 0")
    if max_area is not None and int(max_area) < 0:
        raise ValueError("max_area must be >= 0 (None: the reference's 80 / 25 rule)")
    from . import _lib
    import torch
    lib, dev, stream = device()
    out = states.astype(np.uint8)
    counts = np.zeros((L.shape[0], n_iter, 3), dtype=np.int64)
    for r, a, b, H, W, diag, _ in regions(L):
        area = default_max_area(H) if max_area is None else int(max_area)
        K = int(out[a:b].max()) + 1
        src = torch.from_numpy(out[a:b].copy()).to(dev)
        dst = torch.empty_like(src)
        c = np.zeros(3 * max(n_iter, 1), dtype=np.int64)
        _lib.check(lib.phmrf_smooth_labels(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), H, W, diag, K,
                                           window, area, n_iter, _lib.ptr_i64(c), stream))
        out[a:b] = dst.cpu().numpy()
        counts[r] = c[:3 * n_iter].reshape(n_iter, 3)
        del src, dst
    res = np.asarray(state_vec).copy()
    res.reshape(-1)[:] = out.astype(res.dtype)
    return res, counts


# ---- export ----------------------------------------------------------------------------------------------------------
def _padded(strings):
    """-> uint8 [len(strings), max length], each row one string zero-padded (the strings hold no NUL)"""
    raw = [s.encode() for s in strings]
    width = max(len(s) for s in raw)
    buf = np.zeros((len(raw), width), dtype=np.uint8)
    for k, s in enumerate(raw):
        buf[k, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return buf


def _region_lines(fh, chrom, res, row, states, chunk=1 << 21):
    """the region's lines: per node the bytes of its row bin, its column bin and its state, padding squeezed out"""
    H, W, diag, s1, s2 = int(row[3]), int(row[4]), int(row[8]), int(row[5]), int(row[6])
    first = _padded(["%d\t%d\t%d\t" % (chrom, (s1 + i) * res, (s1 + i + 1) * res) for i in range(H)])
    second = _padded(["%d\t%d\t%d\t" % (chrom, (s2 + j) * res, (s2 + j + 1) * res) for j in range(W)])
    last = _padded(["%d\r\n" % (s + 1) for s in range(MAX_STATES)])
    if diag:
        starts = np.arange(H, dtype=np.int64) * W - np.arange(H, dtype=np.int64) * (np.arange(H, dtype=np.int64) - 1) // 2
    n = states.shape[0]
    for v0 in range(0, n, chunk):
        v = np.arange(v0, min(n, v0 + chunk), dtype=np.int64)
        if diag:
            i = np.searchsorted(starts, v, side="right") - 1
            j = i + (v - starts[i])
        else:
            i, j = v // W, v % W
        mat = np.concatenate([first[i], second[j], last[states[v]]], axis=1)
        fh.write(mat[mat != 0].tobytes())


def write_state_files(state_vec, len_vec, resolution, output_path, annotation):
    """-> the list of files written (see the module's docstring)"""
    states = check_state_vec(state_vec)
    L = check_len_vec(len_vec, states.shape[0])
    res = int(resolution)
    if res < 1:
        raise ValueError("resolution must be >= 1")
    os.makedirs(output_path, exist_ok=True)
    written = []
    for chrom in np.unique(L[:, 9]):
        rows = L[L[:, 9] == chrom]
        name = os.path.join(output_path, "estimate_test%d.%s.txt" % (chrom, annotation))
        with open(name, "wb") as fh:
            for row in rows:
                _region_lines(fh, int(chrom), res, row, states[int(row[1]):int(row[2])])
        written.append(name)
        region = np.zeros((rows.shape[0], 7), dtype=np.int64)
        stop = np.cumsum(rows[:, 2] - rows[:, 1])
        region[:, 0] = rows[:, 2] - rows[:, 1]
        region[:, 1] = stop - region[:, 0] + 1
        region[:, 2] = stop
        region[:, 3:7] = rows[:, [3, 4, 5, 6]]
        name = os.path.join(output_path, "test%d.region.txt" % chrom)
        with open(name, "wb") as fh:
            fh.write("".join("\t".join("%d" % x for x in r) + "\n" for r in region).encode())
        written.append(name)
    return written


def postprocess_file(mat_path, output_path, resolution, window=5, max_area=None, n_iter=1):
    """The command line's --postprocess: smooth the state_vec of a fit (estimate_ou_*.mat) or a segmentation (segment_*.mat),
    write the 'ori' and 'smooth' files of every chromosome and smooth_<stem>.mat.  -> the .mat written"""
    import scipy.io
    d = scipy.io.loadmat(mat_path)
    if "state_vec" not in d or "len_vec" not in d:
        raise ValueError("%s holds no state_vec / len_vec" % mat_path)
    state_vec = check_state_vec(d["state_vec"])
    len_vec = check_len_vec(d["len_vec"], state_vec.shape[0])
    smooth, counts = smooth_states(state_vec, len_vec, window, max_area, n_iter)
    write_state_files(state_vec, len_vec, resolution, output_path, "ori")
    write_state_files(smooth, len_vec, resolution, output_path, "smooth")
    areas = np.array([default_max_area(r[3]) if max_area is None else int(max_area) for r in len_vec], dtype=np.int64)
    out = os.path.join(output_path, "smooth_%s.mat" % stem(mat_path))
    scipy.io.savemat(out, {"state_vec": state_vec, "state_vec_smooth": smooth, "len_vec": len_vec,
                           "smooth_window": int(window), "smooth_area": areas, "smooth_iter": int(n_iter),
                           "smooth_counts": counts, "resolution": int(resolution)})
    return out
