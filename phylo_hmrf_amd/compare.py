"""Comparison of two state maps on the same regions: two cell types or replicates segmented with one
saved model, two repeated fits whose state numbers are permutations of each other, or a map and its smoothed version.

`contingency(a, b)` counts the stored nodes per pair of states on the GPU (phmrf_label_contingency, csrc/compare.hip);
`match_states(C)` renumbers map B's states to map A's by the assignment that maximises the agreement, `scores(C)` gives the
agreement, the adjusted Rand index and the normalised mutual information of a table.  `compare_states(...)` does all of it
region by region and lists the DIFFERENTIAL DOMAINS (phmrf_diff_domains): the 8-connected components, on a region's full
matrix, of the bin pairs where the maps differ and both confidences reach min_conf.  `compare_files(...)` is the command
line's --compare A.mat --compare_with B.mat.

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

from .maps import (CONF_ONE, FIRST_CAPACITY, MAX_STATES, check_len_vec, check_state_vec, conf_array, default_max_area, device,
                   list_rows, regions, stem)

DIFF_BANDS = 32                  # include/phmrf.h PHMRF_DIFF_BANDS
DOMAIN_COLS = 12                 # include/phmrf.h PHMRF_DOMAIN_COLS
CONTINGENCY_GRID_CAP = 1024      # csrc/compare.hip: workgroups of the contingency kernel ...
CONTINGENCY_PER_TRIP = 1024      # ... and the nodes one of them reads per grid-stride trip


def count_pairs(lib, stream, a_t, b_t, KA, KB):
    """-> int64 [KA, KB] of two uint8 device tensors of equal length (phmrf_label_contingency)"""
    from . import _lib
    C = np.zeros(KA * KB, dtype=np.int64)
    _lib.check(lib.phmrf_label_contingency(ctypes.c_void_p(a_t.data_ptr()), ctypes.c_void_p(b_t.data_ptr()), a_t.numel(), KA, KB,
                                           _lib.ptr_i64(C), stream))
    return C.reshape(KA, KB)


def contingency(a, b, KA=None, KB=None):
    """-> int64 [KA, KB]: the number of nodes with state i in a and j in b (K: the largest state + 1 by default)"""
    import torch
    a, b = check_state_vec(a), check_state_vec(b)
    if a.shape != b.shape:
        raise ValueError("the two maps have %d and %d nodes" % (a.size, b.size))
    KA = (int(a.max()) + 1 if a.size else 1) if KA is None else int(KA)
    KB = (int(b.max()) + 1 if b.size else 1) if KB is None else int(KB)
    lib, dev, stream = device()
    if a.size == 0:
        return np.zeros((KA, KB), dtype=np.int64)
    a_t = torch.from_numpy(a.astype(np.uint8)).to(dev)
    b_t = torch.from_numpy(b.astype(np.uint8)).to(dev)
    return count_pairs(lib, stream, a_t, b_t, KA, KB)


def match_states(C):
    """-> map_b uint8 [KB]: B's state j is A's state map_b[j] under the one-to-one assignment with the largest agreement
    (scipy.optimize.linear_sum_assignment); B's unmatched states (KB > KA) take KA, KA + 1, ... in ascending order"""
    from scipy.optimize import linear_sum_assignment
    C = np.asarray(C)
    KA, KB = C.shape
    rows, cols = linear_sum_assignment(C, maximize=True)
    map_b = np.full(KB, -1, dtype=np.int64)
    map_b[cols] = rows
    free = np.nonzero(map_b < 0)[0]
    map_b[free] = KA + np.arange(free.size)
    if map_b.max() >= MAX_STATES:
        raise ValueError("the matched states do not fit %d states" % MAX_STATES)
    return map_b.astype(np.uint8)


def permute_columns(C, map_b):
    """-> the table of A against the renumbered B: column map_b[j] takes column j (last axis)"""
    C = np.asarray(C)
    map_b = np.asarray(map_b, dtype=np.int64)
    out = np.zeros(C.shape[:-1] + (int(map_b.max()) + 1,), dtype=C.dtype)
    np.add.at(out, (Ellipsis, map_b), C)
    return out


def scores(C):
    """-> dict(agreement, ari, nmi) of a contingency table, float64: the share of nodes on the table's diagonal, the
    Hubert-Arabie adjusted Rand index (1.0 when its denominator is 0) and 2 I / (H_A + H_B) (1.0 when both entropies are 0)"""
    C = np.asarray(C, dtype=np.float64)
    n = C.sum()
    if n == 0:
        return dict(agreement=1.0, ari=1.0, nmi=1.0)
    ra, rb = C.sum(axis=1), C.sum(axis=0)
    pairs = lambda x: (x * (x - 1.0) / 2.0).sum()
    s_ab, s_a, s_b, total = pairs(C), pairs(ra), pairs(rb), n * (n - 1.0) / 2.0
    expected = s_a * s_b / total if total > 0 else 0.0
    den = 0.5 * (s_a + s_b) - expected
    ari = 1.0 if den == 0 else float((s_ab - expected) / den)
    p, pa, pb = C / n, ra / n, rb / n
    h = lambda q: float(-(q[q > 0] * np.log(q[q > 0])).sum())
    ha, hb = h(pa), h(pb)
    nz = p > 0
    info = float((p[nz] * np.log(p[nz] / np.outer(pa, pb)[nz])).sum())
    nmi = 1.0 if ha + hb == 0 else 2.0 * info / (ha + hb)
    return dict(agreement=float(np.trace(C) / n), ari=ari, nmi=float(nmi))


def compare_states(state_a, state_b, len_vec, conf_a=None, conf_b=None, match=False, min_conf=0.0, min_area=None):
    """Region by region -> dict:
      contingency [KA, K'], contingency_region [R, KA, K']   nodes per (state in A, state in B after map_b)
      map_b uint8 [KB]                     B's states in A's numbers (the identity unless match)
      agreement, ari, nmi                  scores(contingency); agreement_region [R]
      band_counts int64 [R, 32, 3]         per distance band: nodes, nodes that differ, nodes that differ and count
      diff_vec uint8 [n]                   0 equal, 1 differs below min_conf, 2 differs and counts
      domains int64 [D, 13]                the region's row in len_vec, then the 12 columns of phmrf_diff_domains
      domain_conf float64 [D, 2]           the domains' mean confidences (NaN without confidences)
    min_area=None lists the domains the small-region smoothing would not call small: area >= default_max_area(H) + 1."""
    import torch
    from . import _lib
    a, b = check_state_vec(state_a), check_state_vec(state_b)
    if a.shape != b.shape:
        raise ValueError("the two maps have %d and %d nodes" % (a.size, b.size))
    L = check_len_vec(len_vec, a.shape[0])
    if (conf_a is None) != (conf_b is None):
        raise ValueError("give both confidences or neither")
    min_conf = float(min_conf)
    if min_conf > 0 and conf_a is None:
        raise ValueError("min_conf > 0 needs the confidences of both maps")
    if min_area is not None and int(min_area) < 1:
        raise ValueError("min_area must be >= 1 (None: the smoothing's area rule + 1)")
    n, R = a.shape[0], L.shape[0]
    KA, KB = (int(a.max()) + 1 if n else 1), (int(b.max()) + 1 if n else 1)
    lib, dev, stream = device()
    a_t = torch.from_numpy(a.astype(np.uint8)).to(dev)
    b_t = torch.from_numpy(b.astype(np.uint8)).to(dev)
    ca_t = cb_t = None
    if conf_a is not None:
        ca_t = torch.from_numpy(conf_array(conf_a, n, "conf_a")).to(dev)
        cb_t = torch.from_numpy(conf_array(conf_b, n, "conf_b")).to(dev)
    diff_t = torch.zeros(n, dtype=torch.uint8, device=dev)

    raw = np.stack([count_pairs(lib, stream, a_t[lo:hi], b_t[lo:hi], KA, KB) for _, lo, hi, *_ in regions(L)])
    map_b = match_states(raw.sum(axis=0)) if match else np.arange(KB, dtype=np.uint8)
    per_region = permute_columns(raw, map_b)
    total = per_region.sum(axis=0)

    bands = np.zeros((R, DIFF_BANDS, 3), dtype=np.int64)
    rows = []
    null = ctypes.c_void_p(None)
    for r, lo, hi, H, W, diag, dist0 in regions(L):
        area = default_max_area(H) + 1 if min_area is None else int(min_area)

        def call(capacity, table, found):
            _lib.check(lib.phmrf_diff_domains(
                ctypes.c_void_p(a_t[lo:hi].data_ptr()), ctypes.c_void_p(b_t[lo:hi].data_ptr()),
                map_b.ctypes.data_as(ctypes.c_void_p), null if ca_t is None else ctypes.c_void_p(ca_t[lo:hi].data_ptr()),
                null if cb_t is None else ctypes.c_void_p(cb_t[lo:hi].data_ptr()), H, W, diag, dist0, KA, KB,
                min_conf, area, ctypes.c_void_p(diff_t[lo:hi].data_ptr()), capacity, _lib.ptr_i64(table), ctypes.byref(found),
                _lib.ptr_i64(bands[r]), stream))

        table = list_rows(call, DOMAIN_COLS, FIRST_CAPACITY)
        rows.append(np.concatenate([np.full((table.shape[0], 1), r, dtype=np.int64), table], axis=1))
    domains = np.concatenate(rows) if rows else np.zeros((0, DOMAIN_COLS + 1), dtype=np.int64)
    if conf_a is None:
        domain_conf = np.full((domains.shape[0], 2), np.nan)
    else:
        domain_conf = domains[:, 10:12].astype(np.float64) / (domains[:, 6:7].astype(np.float64) * CONF_ONE)
    nodes = per_region.sum(axis=(1, 2)).astype(np.float64)
    res = dict(contingency=total, contingency_region=per_region, map_b=map_b, band_counts=bands,
               agreement_region=np.trace(per_region, axis1=1, axis2=2) / np.where(nodes > 0, nodes, 1.0),
               diff_vec=diff_t.cpu().numpy(), domains=domains, domain_conf=domain_conf)
    res.update(scores(total))
    return res


def domain_lines(domains, domain_conf, len_vec, resolution):
    """-> the lines of compare_domains_*.txt, header first: the bounding boxes in genome coordinates, states 1-based"""
    res = int(resolution)
    lines = ["#chrom\tstart1\tstop1\tstart2\tstop2\tarea\tnodes\tstateA\tstateB\tconfA\tconfB\n"]
    for d, c in zip(np.asarray(domains), np.asarray(domain_conf)):
        row = len_vec[int(d[0])]
        s1, s2 = int(row[5]), int(row[6])
        lines.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t%.6f\n"
                     % (row[9], (s1 + d[2]) * res, (s1 + d[3] + 1) * res, (s2 + d[4]) * res, (s2 + d[5] + 1) * res, d[7], d[6],
                        d[8] + 1, d[9] + 1, c[0], c[1]))
    return lines


def load_pair(path_a, path_b, field="state_vec", min_conf=0.0):
    """The two files' states, their common len_vec and, when both hold one, their confidences; ValueError for files that
    cannot be compared.  Host only."""
    import scipy.io
    da, db = scipy.io.loadmat(path_a), scipy.io.loadmat(path_b)
    for path, d in ((path_a, da), (path_b, db)):
        if field not in d or "len_vec" not in d:
            raise ValueError("%s holds no %s / len_vec" % (path, field))
    sa, sb = check_state_vec(da[field]), check_state_vec(db[field])
    la, lb = check_len_vec(da["len_vec"], sa.shape[0]), check_len_vec(db["len_vec"], sb.shape[0])
    if la.shape[0] != lb.shape[0] or not np.array_equal(la[:, :10], lb[:, :10]):
        raise ValueError("%s and %s do not hold the same regions (len_vec columns 0 - 9 differ)" % (path_a, path_b))
    both = "conf" in da and "conf" in db
    if float(min_conf) > 0 and not both:
        raise ValueError("--compare_min_conf %g needs a conf in both files (segment_*.mat)" % float(min_conf))
    conf = (np.asarray(da["conf"]).reshape(-1), np.asarray(db["conf"]).reshape(-1)) if both else (None, None)
    return sa, sb, la, conf


def compare_files(path_a, path_b, output_path, resolution, field="state_vec", match=False, min_conf=0.0, min_area=None):
    """The command line's --compare: compare the `field` of two estimate_ou_*.mat / segment_*.mat / smooth_*.mat on the same
    regions, write compare_<stemA>__<stemB>.mat and compare_domains_<stemA>__<stemB>.txt under output_path.  -> the .mat"""
    import scipy.io
    if int(resolution) < 1:
        raise ValueError("resolution must be >= 1")
    sa, sb, L, (ca, cb) = load_pair(path_a, path_b, field, min_conf)
    res = compare_states(sa, sb, L, ca, cb, match=bool(match), min_conf=min_conf, min_area=min_area)
    os.makedirs(output_path, exist_ok=True)
    name = "%s__%s" % (stem(path_a), stem(path_b))
    areas = np.array([default_max_area(r[3]) + 1 if min_area is None else int(min_area) for r in L], dtype=np.int64)
    out = os.path.join(output_path, "compare_%s.mat" % name)
    scipy.io.savemat(out, dict(res, len_vec=L, compare_field=field, compare_match=int(bool(match)),
                               compare_min_conf=float(min_conf), compare_area=areas, resolution=int(resolution)))
    with open(os.path.join(output_path, "compare_domains_%s.txt" % name), "wb") as fh:
        fh.write("".join(domain_lines(res["domains"], res["domain_conf"], L, resolution)).encode())
    return out
