"""The pile-up of a state map around centres restated as the definition reads (what the GPU's
phmrf_state_pileup and phylo_hmrf_amd.pileup.state_pileup are held to): build the full matrix, loop over the centres and the
pile cells.  Host only, shares nothing with phylo_hmrf_amd.pileup."""
import numpy as np


def full_matrix(labels, H, W, diag):
    """-> int64 [H, W]: the block itself, or the symmetric matrix of a diagonal block's stored nodes"""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    if not diag:
        return lab.reshape(H, W)
    M = np.zeros((H, H), dtype=np.int64)
    M[np.triu_indices(H)] = lab
    return M + M.T - np.diag(np.diag(M))


def pile(M, K, w, G, groups, ci, cj, orient):
    """M [H, W] with -1 on the cells that count for nothing -> obs int64 [G, 2w + 1, 2w + 1, K]; centre t is (ci[t], cj[t],
    orient[t]) of group groups[t]"""
    H, W = M.shape
    obs = np.zeros((G, 2 * w + 1, 2 * w + 1, K), dtype=np.int64)
    for t in range(len(ci)):
        flip, transpose = int(orient[t]) & 1, int(orient[t]) & 2
        for u in range(-w, w + 1):
            for v in range(-w, w + 1):
                p, q = (v, u) if transpose else (u, v)
                s = -1 if flip else 1
                i, j = int(ci[t]) + s * p, int(cj[t]) + s * q
                if 0 <= i < H and 0 <= j < W and M[i, j] >= 0:
                    assert M[i, j] < K, (i, j, M[i, j])
                    obs[int(groups[t]), u + w, v + w, M[i, j]] += 1
    return obs


def table(labels, H, W, diag, K, w, G, offsets, ci, cj, orient=None):
    """-> obs int64 [G, 2w + 1, 2w + 1, K] of one region; the centres of group g are the entries [offsets[g], offsets[g + 1])"""
    n = int(offsets[G])
    groups = np.repeat(np.arange(G), np.diff(np.asarray(offsets)[:G + 1]))
    return pile(full_matrix(labels, H, W, diag), K, w, G, groups, ci[:n], cj[:n], np.zeros(n, dtype=np.int64) if orient is None else orient[:n])


def chromosome_matrix(state_vec, len_vec, chrom):
    """-> int64 [B, B]: the symmetric matrix of the chromosome assembled from all of its regions, -1 where nothing covers"""
    s, L = np.asarray(state_vec).reshape(-1), np.asarray(len_vec)
    rows = [r for r in L if int(r[9]) == chrom]
    B = max(max(int(r[5] + r[3]), int(r[6] + r[4])) for r in rows)
    C = np.full((B, B), -1, dtype=np.int64)
    for r in rows:
        a, b, H, W, s1, s2, diag = (int(r[x]) for x in (1, 2, 3, 4, 5, 6, 8))
        M = full_matrix(s[a:b], H, W, bool(diag))
        C[s1:s1 + H, s2:s2 + W] = M
        C[s2:s2 + W, s1:s1 + H] = M.T
    return C


def state_pileup(state_vec, len_vec, centres, w, K, G):
    """centres rows chrom, bin_a, bin_b, group, orient -> obs int64 [G, 2w + 1, 2w + 1, K] piled on the chromosomes' matrices"""
    c = np.asarray(centres).reshape(-1, 5)
    obs = np.zeros((G, 2 * w + 1, 2 * w + 1, K), dtype=np.int64)
    for chrom in np.unique(np.asarray(len_vec)[:, 9]):
        sel = c[c[:, 0] == chrom]
        obs += pile(chromosome_matrix(state_vec, len_vec, int(chrom)), K, w, G, sel[:, 3], sel[:, 1], sel[:, 2], sel[:, 4])
    return obs
