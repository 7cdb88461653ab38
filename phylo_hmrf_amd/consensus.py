"""The consensus of several state maps on the same regions: repeated fits under different seeds, or one
saved model applied to several replicates and cell types.

`consensus_states(maps, len_vec, ...)` votes, region by region, on the GPU (phmrf_label_consensus, csrc/consensus.hip): per
stored node the CONSENSUS is the state most maps hold, the lowest on ties, its SUPPORT the number of maps that hold it.  With
it come the tables that say how the maps stand to the ensemble: support_hist (nodes per consensus state and support), agree
(per map its contingency table against the consensus), pair (nodes on which two maps agree) and the counts per distance band.
With `match` the state numbers of the maps 1 .. M - 1 are first brought to map 0's by compare.match_states.
`consensus_files(...)` is the command line's --consensus A.mat,B.mat,...: its consensus_*.mat loads back through
maps.load_map with conf = support / M, so every reader of one state map takes the ensemble as its input.

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

from .compare import DIFF_BANDS, count_pairs, match_states, scores
from .maps import MAX_STATES, check_len_vec, check_state_vec, default_max_area, device, load_map, regions, stem

CONSENSUS_MAPS = 16              # include/phmrf.h PHMRF_CONSENSUS_MAPS
CONSENSUS_GRID_CAP = 1024        # csrc/consensus.hip: workgroups of the vote kernel ...
CONSENSUS_PER_TRIP = 1024        # ... the nodes one of them takes per grid-stride trip ...
CONSENSUS_AGREE_BINS = 8192      # ... and the bins of agree it holds: maps beyond 8192 // K^2 go through the chunk kernel
NOT_A_STATE = 255                # renumber[m][l] of a raw label l that map m does not hold
FIELDS = ("state_vec", "state_vec_smooth")


def majority(M):
    """the strict majority of M maps"""
    return int(M) // 2 + 1


def check_support(min_support, M):
    """-> min_support as an int in [1, M] (None: the strict majority)"""
    s = majority(M) if min_support is None else int(min_support)
    if not 1 <= s <= M:
        raise ValueError("min_support %d is outside [1, %d], the number of maps" % (s, M))
    return s


def check_maps(maps):
    """-> the maps as int64 [M, n]: 1 .. CONSENSUS_MAPS state vectors of equal length"""
    maps = [check_state_vec(m) for m in maps]
    if not 1 <= len(maps) <= CONSENSUS_MAPS:
        raise ValueError("a consensus takes 1 .. %d maps, not %d" % (CONSENSUS_MAPS, len(maps)))
    for m, v in enumerate(maps):
        if v.shape != maps[0].shape:
            raise ValueError("map 0 and map %d have %d and %d nodes" % (m, maps[0].size, v.size))
    return np.stack(maps)


def identity_table(M, K):
    """-> renumber uint8 [M, 64]: raw state l < K is state l, any other label is NOT_A_STATE"""
    ren = np.full((M, MAX_STATES), NOT_A_STATE, dtype=np.uint8)
    ren[:, :K] = np.arange(K, dtype=np.uint8)
    return ren


def matched_table(tables, K0):
    """-> renumber uint8 [M, 64] from tables[m - 1] = the contingency table [K0, K_m] of map 0 against map m: map 0 keeps its
    numbers, map m's state l is map 0's state match_states(table)[l]; a state that match_states leaves unmatched takes the
    next number no map has used yet (two maps' left-over states are never merged).  ValueError beyond 64 states.  Host only."""
    M = len(tables) + 1
    ren = np.full((M, MAX_STATES), NOT_A_STATE, dtype=np.uint8)
    ren[0, :K0] = np.arange(K0, dtype=np.uint8)
    free = K0
    for m, C in enumerate(tables, start=1):
        to = match_states(C).astype(np.int64)
        for l in np.nonzero(to >= K0)[0]:
            to[l] = free
            free += 1
        if free > MAX_STATES:
            raise ValueError("the matched maps hold more than %d states between them" % MAX_STATES)
        ren[m, :to.size] = to
    return ren


def map_scores(agree):
    """-> dict(agreement, ari, nmi), float64 [M] each: compare.scores of every map's table against the consensus"""
    got = [scores(a) for a in np.asarray(agree)]
    return dict((k, np.array([g[k] for g in got], dtype=np.float64)) for k in ("agreement", "ari", "nmi"))


def consensus_states(maps, len_vec, match=False, min_support=None, K=None):
    """Region by region -> dict:
      state_vec uint8 [n]                 the consensus: the most voted state, the lowest on ties
      support uint8 [n], conf float32 [n] the maps that hold it, and that number over M
      core_vec uint8 [n] or None          the consensus where support >= min_support, else K ("unstable"); None at K = 64
      renumber uint8 [M, 64]              raw state l of map m counts as renumber[m][l] (255: not a state of the map)
      support_hist [K, M + 1], support_hist_region [R, K, M + 1]   nodes per (consensus, support)
      agree int64 [M, K, K]               agree[m][c][a]: nodes with consensus c whose map m holds a
      pair int64 [M, M], pair_agreement float64 [M, M]   nodes on which two maps agree, and that over n
      agreement, ari, nmi float64 [M]     compare.scores(agree[m]): every map against the consensus
      band_counts int64 [R, 32, 3]        per distance band: nodes, nodes with support >= min_support, unanimous nodes
      K, M, min_support
    min_support=None: the strict majority M // 2 + 1.  With match every map m >= 1 is renumbered to map 0 (matched_table)."""
    import torch
    from . import _lib
    S = check_maps(maps)
    M, n = S.shape
    L = check_len_vec(len_vec, n)
    min_support = check_support(min_support, M)
    lib, dev, stream = device()
    S_t = torch.from_numpy(S.astype(np.uint8)).to(dev)
    tops = [int(v.max()) + 1 for v in S]                 # (a checked len_vec has a region, a region a node)
    if match:
        ren = matched_table([count_pairs(lib, stream, S_t[0], S_t[m], tops[0], tops[m]) for m in range(1, M)], tops[0])
        need = int(ren[ren != NOT_A_STATE].max()) + 1
    else:
        need = max(tops)
        ren = None
    K = need if K is None else int(K)
    if not need <= K <= MAX_STATES:
        raise ValueError("K = %d does not hold the maps' %d states (at most %d)" % (K, need, MAX_STATES))
    if ren is None:
        ren = identity_table(M, K)

    R = L.shape[0]
    cons_t = torch.zeros(n, dtype=torch.uint8, device=dev)
    sup_t = torch.zeros(n, dtype=torch.uint8, device=dev)
    core_t = torch.zeros(n, dtype=torch.uint8, device=dev) if K < MAX_STATES else None
    hist = np.zeros((R, K, M + 1), dtype=np.int64)
    agree = np.zeros((R, M, K, K), dtype=np.int64)
    pair = np.zeros((R, M, M), dtype=np.int64)
    bands = np.zeros((R, DIFF_BANDS, 3), dtype=np.int64)
    null = ctypes.c_void_p(None)
    for r, lo, hi, H, W, diag, dist0 in regions(L):
        ptrs = (ctypes.c_void_p * M)(*[S_t[m, lo:hi].data_ptr() for m in range(M)])
        _lib.check(lib.phmrf_label_consensus(
            ctypes.cast(ptrs, ctypes.c_void_p), M, ren.ctypes.data_as(ctypes.c_void_p) if match else null, K, H, W, diag, dist0,
            min_support, ctypes.c_void_p(cons_t[lo:hi].data_ptr()), ctypes.c_void_p(sup_t[lo:hi].data_ptr()),
            null if core_t is None else ctypes.c_void_p(core_t[lo:hi].data_ptr()), _lib.ptr_i64(hist[r]), _lib.ptr_i64(agree[r]),
            _lib.ptr_i64(pair[r]), _lib.ptr_i64(bands[r]), stream))
    support = sup_t.cpu().numpy()
    total_agree, total_pair = agree.sum(axis=0), pair.sum(axis=0)
    res = dict(state_vec=cons_t.cpu().numpy(), support=support, conf=support.astype(np.float32) / np.float32(M),
               core_vec=None if core_t is None else core_t.cpu().numpy(), renumber=ren, support_hist=hist.sum(axis=0),
               support_hist_region=hist, agree=total_agree, pair=total_pair, pair_agreement=total_pair / float(n),
               band_counts=bands, K=K, M=M, min_support=min_support)
    res.update(map_scores(total_agree))
    return res


def summary_lines(res, paths):
    """-> the lines of consensus_*.txt: per map its path, agreement, ARI and NMI against the consensus and the mean of its
    pair_agreement row without the diagonal (1.0 for a single map); per state (1-based) its nodes, mean support and the shares
    of its nodes that are unanimous and stable (support >= min_support); 0 for a state the consensus never takes"""
    M, K, ms = int(res["M"]), int(res["K"]), int(res["min_support"])
    pa = np.asarray(res["pair_agreement"], dtype=np.float64).reshape(M, M)
    hist = np.asarray(res["support_hist"], dtype=np.int64).reshape(K, M + 1)
    lines = ["#map\tpath\tagreement\tari\tnmi\tmean_pair_agreement\n"]
    for m in range(M):
        others = (pa[m].sum() - pa[m, m]) / (M - 1) if M > 1 else 1.0
        lines.append("%d\t%s\t%.6f\t%.6f\t%.6f\t%.6f\n" % (m + 1, paths[m], np.ravel(res["agreement"])[m], np.ravel(res["ari"])[m],
                                                         np.ravel(res["nmi"])[m], others))
    lines.append("#state\tnodes\tmean_support\tunanimous\tstable\n")
    for k in range(K):
        nodes = int(hist[k].sum())
        den = float(max(nodes, 1))
        votes = float((hist[k] * np.arange(M + 1)).sum())
        lines.append("%d\t%d\t%.6f\t%.6f\t%.6f\n" % (k + 1, nodes, votes / den, hist[k, M] / den, hist[k, ms:].sum() / den))
    return lines


def save_mat(path, res, len_vec, paths, resolution, field="state_vec", match=False, min_area=None):
    """write consensus_*.mat: the result (no core_vec at K = 64), len_vec and the settings.  Host only."""
    import scipy.io
    areas = np.array([default_max_area(r[3]) + 1 if min_area is None else int(min_area) for r in len_vec], dtype=np.int64)
    out = dict((k, v) for k, v in res.items() if v is not None)
    out.update(len_vec=len_vec, consensus_files=np.array([str(p) for p in paths], dtype=object), consensus_field=field,
               consensus_match=int(bool(match)), consensus_area=areas, resolution=int(resolution))
    scipy.io.savemat(path, out)


def load_all(paths, field="state_vec"):
    """-> (the files' states, their common len_vec); ValueError for fewer than two or more than CONSENSUS_MAPS files, a field
    that is no state vector, or two files that do not hold the same regions.  Host only."""
    paths = list(paths)
    if field not in FIELDS:
        raise ValueError("field must be state_vec or state_vec_smooth, not %r" % (field,))
    if not 2 <= len(paths) <= CONSENSUS_MAPS:
        raise ValueError("a consensus takes 2 .. %d files, not %d" % (CONSENSUS_MAPS, len(paths)))
    states, first = [], None
    for p in paths:
        s, L, _ = load_map(p, field)
        if first is None:
            first = L
        elif L.shape[0] != first.shape[0] or not np.array_equal(L[:, :10], first[:, :10]):
            raise ValueError("%s and %s do not hold the same regions (len_vec columns 0 - 9 differ)" % (paths[0], p))
        states.append(s)
    return states, first


def consensus_files(paths, output_path, resolution, field="state_vec", match=False, min_support=None, min_area=None):
    """The command line's --consensus: vote on the `field` of the .mat files, write consensus_<stem of the first>_<M>.mat,
    consensus_<...>.txt (summary_lines) and, unless K = 64, consensus_domains_<...>.txt: the domains of core_vec
    (domains.state_domains with conf = support / M; state K + 1 there is "unstable").  -> the .mat"""
    if int(resolution) < 1:
        raise ValueError("resolution must be >= 1")
    if min_area is not None and int(min_area) < 1:
        raise ValueError("min_area must be >= 1 (None: the smoothing's area rule + 1)")
    paths = list(paths)
    states, L = load_all(paths, field)
    min_support = check_support(min_support, len(paths))
    res = consensus_states(states, L, match=bool(match), min_support=min_support)
    os.makedirs(output_path, exist_ok=True)
    name = "%s_%d" % (stem(paths[0]), len(paths))
    out = os.path.join(output_path, "consensus_%s.mat" % name)
    save_mat(out, res, L, paths, resolution, field, match, min_area)
    with open(os.path.join(output_path, "consensus_%s.txt" % name), "wb") as fh:
        fh.write("".join(summary_lines(res, paths)).encode())
    if res["core_vec"] is not None:
        from .domains import domain_lines, state_domains
        dom = state_domains(res["core_vec"], L, res["conf"], min_area=min_area)
        with open(os.path.join(output_path, "consensus_domains_%s.txt" % name), "wb") as fh:
            fh.write("".join(domain_lines(dom["domains"], dom["domain_conf"], L, resolution)).encode())
    return out
