"""What the post-processing modules share (smooth, compare, domains, tracks, render, enrich, pileup, query, aggregate): the
checks of a state map, its regions and its number of states, the walk over the regions, the lines of an annotation file, the
GPU handle and the protocol of the calls that list rows; what only the modes that read a list of intervals share is in
intervals.py.  Host only apart from `device()`.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

MAX_STATES = 64                  # K <= 64 in every post-processing call (u8 labels, 64-bin histograms)
FIRST_CAPACITY = 65536           # rows of a region's first listing call; a second call takes the count the first returned
CONF_ONE = float(1 << 24)        # the fixed point of the confidence sums


def default_max_area(H):
    """read_state_test.m: threshold 80, or 25 when the region's height (len_vec column 4) is < 100"""
    return 25 if int(H) < 100 else 80


def _integral(a, what):
    a = np.asarray(a)
    if a.dtype.kind in "iu":
        return a.astype(np.int64)
    if a.dtype.kind == "f" and a.size and np.all(np.isfinite(a)) and np.all(a == np.round(a)):
        return a.astype(np.int64)
    if a.dtype.kind == "f" and a.size == 0:
        return a.astype(np.int64)
    raise ValueError("%s must hold integers (got dtype %s)" % (what, a.dtype))


def check_state_vec(state_vec):
    """-> the states as int64 [n] (any shape with one non-singleton axis; a .mat file stores them as 1 x n)"""
    s = _integral(state_vec, "state_vec").reshape(-1)
    if s.size and (s.min() < 0 or s.max() >= MAX_STATES):
        raise ValueError("state_vec must hold states in [0, %d) (got %d .. %d)" % (MAX_STATES, s.min(), s.max()))
    return s


def check_K(s, K):
    """-> K: the largest state of the checked states s + 1 by default (1 without any), in 1 .. MAX_STATES"""
    K = (int(s.max()) + 1 if s.size else 1) if K is None else int(K)
    if K < 1 or K > MAX_STATES:
        raise ValueError("K must be in 1 .. %d" % MAX_STATES)
    return K


def check_len_vec(len_vec, n_states):
    """-> len_vec as int64 [regions, >= 10]; every region a consistent slice of a state_vec of n_states entries"""
    L = _integral(np.atleast_2d(len_vec), "len_vec")
    if L.ndim != 2 or L.shape[1] < 10 or L.shape[0] < 1:
        raise ValueError("len_vec must have rows of at least 10 columns (got shape %s)" % (L.shape,))
    for r, row in enumerate(L):
        n, a, b, H, W, diag = (int(x) for x in row[[0, 1, 2, 3, 4, 8]])
        if H < 1 or W < 1 or diag not in (0, 1) or (diag == 1 and H != W):
            raise ValueError("len_vec row %d: H = %d, W = %d, type %d is not a region" % (r, H, W, diag))
        want = H * (H + 1) // 2 if diag else H * W
        if not (0 <= a <= b <= n_states) or b - a != want or n != want:
            raise ValueError("len_vec row %d: [%d, %d) with n = %d does not hold the %d nodes of a %s %d x %d region of a "
                             "state_vec of %d" % (r, a, b, n, want, "diagonal" if diag else "off-diagonal", H, W, n_states))
        if row[5] < 0 or row[6] < 0:
            raise ValueError("len_vec row %d: negative start bin" % r)
    return L


def regions(len_vec):
    """yields (r, lo, hi, H, W, diag, dist0) per row of a checked len_vec: the region's slice [lo, hi) of the state_vec, its
    shape and type, and the distance start_bin2 - start_bin1 of its cell (0, 0)"""
    for r, row in enumerate(len_vec):
        yield r, int(row[1]), int(row[2]), int(row[3]), int(row[4]), int(row[8]), int(row[6]) - int(row[5])


def conf_array(conf, n, what):
    """-> conf as contiguous float32 [n]"""
    c = np.ascontiguousarray(np.asarray(conf, dtype=np.float32).reshape(-1))
    if c.shape[0] != n:
        raise ValueError("%s has %d entries for %d nodes" % (what, c.shape[0], n))
    return c


def stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def chrom_of(text):
    """the chromosome number of `chr<N>` or `<N>` in an annotation file (len_vec's column 9), None for any other name"""
    t = text[3:] if text.startswith("chr") else text
    return int(t) if t.isdigit() else None


def is_number(text):
    """a field of an annotation file that reads as an integer, with a sign at most"""
    return text.lstrip("-").isdigit() and text.count("-") <= 1


def annotation_lines(path):
    """yields (line number from 1, the line, its fields) of a BED / BEDPE file, separated by tabs or spaces, without the
    blank lines and those that start with #"""
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            f = line.split()
            if f and not f[0].startswith("#"):
                yield number, line.rstrip("\n"), f


def check_resolution(resolution):
    res = int(resolution)
    if res < 1:
        raise ValueError("resolution must be >= 1")
    return res


def load_map(path, field="state_vec"):
    """-> (states, len_vec, conf or None) of an estimate_ou_*.mat / segment_*.mat / smooth_*.mat.  Host only."""
    import scipy.io
    d = scipy.io.loadmat(path)
    if field not in d or "len_vec" not in d:
        raise ValueError("%s holds no %s / len_vec" % (path, field))
    s = check_state_vec(d[field])
    return s, check_len_vec(d["len_vec"], s.shape[0]), (np.asarray(d["conf"]).reshape(-1) if "conf" in d else None)


def device():
    """-> (the library, the current torch device, its current stream as a c_void_p); an error without a GPU"""
    from . import _lib
    import torch
    lib = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    return lib, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def list_rows(call, cols, first=FIRST_CAPACITY):
    """The two-call protocol of phmrf_diff_domains / phmrf_state_domains: call(capacity, table, found) runs the entry point
    with an int64 [max(capacity, 1), cols] table and a c_int64 for the count.  `first` rows to begin with; if the region holds
    more, once more with the count the first call returned.  -> the rows found, int64 [found, cols]"""
    def run(capacity):
        table = np.zeros((max(capacity, 1), cols), dtype=np.int64)
        found = ctypes.c_int64(0)
        call(capacity, table, found)
        return table, int(found.value)

    table, found = run(first)
    if found > first:
        table, found = run(found)
    return table[:found]
