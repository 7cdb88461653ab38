"""The rescaled pile-up of a state map over features of unequal size restated as the definition reads (DESIGN.md section 7;
what the GPU's phmrf_state_aggregate and phylo_hmrf_amd.aggregate.state_aggregate are held to): form the bin pair of every
stored node of every region, loop over the features and the pile cells, count both orientations, vote with np.argmax.  Host
only.  It shares no code with phylo_hmrf_amd/aggregate.py except axis_cells, which tests/test_aggregate_cpu.py pins by hand."""
import numpy as np

from phylo_hmrf_amd.aggregate import axis_cells


def node_pairs(row):
    """-> (p, q): the bin pair (start_bin1 + i, start_bin2 + j) of every stored node of a region in storage order"""
    H, W, s1, s2, diag = (int(row[x]) for x in (3, 4, 5, 6, 8))
    if diag:
        I, J = np.triu_indices(H)
    else:
        I, J = np.divmod(np.arange(H * W), W)
    return I.astype(np.int64) + s1, J.astype(np.int64) + s2


def feature_hist(state_vec, len_vec, feature, T, F, K):
    """-> hist int64 [P, P, K] of one feature (chrom, a0, a1, b0, b1, group, flip); a state >= K inside a cell is an
    AssertionError"""
    s, L = np.asarray(state_vec).astype(np.int64).reshape(-1), np.asarray(len_vec, dtype=np.int64)
    chrom, a0, a1, b0, b1, _, flip = (int(x) for x in feature)
    P = T + 2 * F
    alo, ahi = axis_cells(a0, a1, T, F)
    blo, bhi = axis_cells(b0, b1, T, F)
    hist = np.zeros((P, P, K), dtype=np.int64)
    for row in L:
        if int(row[9]) != chrom:
            continue
        p, q = node_pairs(row)
        lab = s[int(row[1]):int(row[2])]
        for u in range(P):
            uu = P - 1 - u if flip else u
            near = ((alo[uu] <= p) & (p < ahi[uu])) | ((alo[uu] <= q) & (q < ahi[uu]))      # only these nodes can be in row u
            if not near.any():
                continue
            pu, qu, labu = p[near], q[near], lab[near]
            p_in_i, q_in_i = (alo[uu] <= pu) & (pu < ahi[uu]), (alo[uu] <= qu) & (qu < ahi[uu])
            for v in range(P):
                vv = P - 1 - v if flip else v
                p_in_j, q_in_j = (blo[vv] <= pu) & (pu < bhi[vv]), (blo[vv] <= qu) & (qu < bhi[vv])
                for inside in (p_in_i & q_in_j, (pu != qu) & q_in_i & p_in_j):
                    if inside.any():
                        assert labu[inside].max() < K, (u, v, labu[inside].max())
                        hist[u, v] += np.bincount(labu[inside], minlength=K)
    return hist


def state_aggregate(state_vec, len_vec, features, T, F, K, G):
    """features rows chrom, a0, a1, b0, b1, group, flip -> (cells, votes), int64 [G, P, P, K] each"""
    P = T + 2 * F
    cells = np.zeros((G, P, P, K), dtype=np.int64)
    votes = np.zeros_like(cells)
    for feature in np.asarray(features, dtype=np.int64).reshape(-1, 7):
        hist = feature_hist(state_vec, len_vec, feature, T, F, K)
        g = int(feature[5])
        cells[g] += hist
        full = hist.sum(axis=-1) > 0
        uu, vv = np.nonzero(full)
        votes[g, uu, vv, np.argmax(hist, axis=-1)[full]] += 1      # (np.argmax: the lowest index on ties)
    return cells, votes
