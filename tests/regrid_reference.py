"""A state map resampled onto another grid restated as the definition reads (what the GPU's
phmrf_regrid_states and phylo_hmrf_amd.regrid.regrid_states are held to): per chromosome the dense count planes [K][B][B] of
the full source matrix from every region's stored nodes in both orientations, then a loop over target cells and source cells
with the overlap written out in Python integers, and a vote with np.argmax.  Host only.  It shares no code with
phylo_hmrf_amd/regrid.py.  The builders of small maps that the regrid tests share are at the end."""
import numpy as np


def ov(x, p, a, b):
    """the units target bin x = [x b, (x + 1) b) and source bin p = [p a, (p + 1) a) share"""
    lo, hi = max(x * b, p * a), min((x + 1) * b, (p + 1) * a)
    return hi - lo if hi > lo else 0


def planes(state_vec, len_vec, chrom, K):
    """-> (C int64 [K, B, B], bad bool [B, B]): C[k][p][q] = the stored nodes of the chromosome's regions in state k that stand
    for (p, q), an off-diagonal node for (q, p) too; bad: a node there has a state >= K.  B: one past the last bin held."""
    s, L = np.asarray(state_vec).astype(np.int64).reshape(-1), np.asarray(len_vec, dtype=np.int64)
    rows = [r for r in L if int(r[9]) == chrom]
    B = max([1] + [max(int(r[5]) + int(r[3]), int(r[6]) + int(r[4])) for r in rows])
    C, bad = np.zeros((K, B, B), dtype=np.int64), np.zeros((B, B), dtype=bool)
    for r in rows:
        lo, H, W, s1, s2, diag = (int(r[x]) for x in (1, 3, 4, 5, 6, 8))
        v = lo
        for i in range(H):
            for j in range(i if diag else 0, W):
                p, q, k = s1 + i, s2 + j, int(s[v])
                v += 1
                for (x, y) in ((p, q),) if p == q else ((p, q), (q, p)):
                    if k >= K:
                        bad[x, y] = True
                    else:
                        C[k, x, y] += 1
    return C, bad


def cell_votes(C, bad, a, b, x, y):
    """-> votes int64 [K] of the target bin pair (x, y); ValueError when a source cell it reads is bad"""
    K, B = C.shape[0], C.shape[1]
    votes = np.zeros(K, dtype=np.int64)
    for p in range((x * b) // a, min(B, -(-((x + 1) * b) // a))):
        wp = ov(x, p, a, b)
        for q in range((y * b) // a, min(B, -(-((y + 1) * b) // a))):
            w = wp * ov(y, q, a, b)
            if w == 0:
                continue
            if bad[p, q]:
                raise ValueError("a label >= K inside the read cell (%d, %d)" % (x, y))
            votes += w * C[:, p, q]
    return votes


def regrid_region(C, bad, a, b, H, W, diag, t1, t2, min_cover, fill):
    """one target region -> (state u8 [n_t], support u32 [n_t], covered u32 [n_t], hist int64 [K + 1], mixed) in node order"""
    K = C.shape[0]
    state, support, covered = [], [], []
    hist, mixed = np.zeros(K + 1, dtype=np.int64), 0
    for i in range(H):
        for j in range(i if diag else 0, W):
            votes = cell_votes(C, bad, a, b, t1 + i, t2 + j)
            cov, k = int(votes.sum()), int(np.argmax(votes))                 # (np.argmax: the lowest index on ties)
            sup = int(votes[k])
            called = cov >= min_cover
            state.append(k if called else fill)
            support.append(sup)
            covered.append(cov)
            hist[k if called else K] += 1
            mixed += 1 if called and sup < cov else 0
    return np.array(state, dtype=np.uint8), np.array(support, dtype=np.uint32), np.array(covered, dtype=np.uint32), hist, mixed


def regrid(state_vec, len_vec, dst_len_vec, a, b, K, min_cover, fill=None):
    """every target region -> dict(state_vec, support, covered, hist_region, mixed_region); n = the largest stop"""
    D = np.asarray(dst_len_vec, dtype=np.int64)
    fill = K if fill is None else fill
    n = int(D[:, 2].max())
    state, support, covered = np.full(n, fill, dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    hist_region, mixed_region = np.zeros((D.shape[0], K + 1), dtype=np.int64), np.zeros(D.shape[0], dtype=np.int64)
    cache = {}
    for t, row in enumerate(D):
        lo, hi, H, W, t1, t2, diag, chrom = (int(row[x]) for x in (1, 2, 3, 4, 5, 6, 8, 9))
        if chrom not in cache:
            cache[chrom] = planes(state_vec, len_vec, chrom, K)
        C, bad = cache[chrom]
        state[lo:hi], support[lo:hi], covered[lo:hi], hist_region[t], mixed_region[t] = regrid_region(
            C, bad, a, b, H, W, diag, t1, t2, min_cover, fill)
    return dict(state_vec=state, support=support, covered=covered, hist_region=hist_region, mixed_region=mixed_region)


# ---- small maps -------------------------------------------------------------------------------------------------------------
def len_vec_of(regions):
    """regions: (H, W, start_bin1, start_bin2, diagonal, chrom) -> len_vec int64 [R, 10], the nodes back to back"""
    rows, at = [], 0
    for r, (H, W, s1, s2, diag, chrom) in enumerate(regions):
        n = H * (H + 1) // 2 if diag else H * W
        rows.append([n, at, at + n, H, W, s1, s2, r, diag, chrom])
        at += n
    return np.array(rows, dtype=np.int64)


def state_vec_of(L, matrices):
    """matrices: chrom -> the symmetric bin x bin matrix of the chromosome -> the stored nodes of every region of L"""
    parts = []
    for row in L:
        H, W, s1, s2, diag, chrom = (int(row[x]) for x in (3, 4, 5, 6, 8, 9))
        M = matrices[chrom][s1:s1 + H, s2:s2 + W]
        parts.append(M[np.triu_indices(H)] if diag else M.reshape(-1))
    return np.concatenate(parts).astype(np.int64)


def symmetric(B, K, seed, blocky=False):
    """a symmetric B x B matrix of states below K; blocky: constant tiles of 1 - 9 bins a side"""
    rng = np.random.default_rng(seed)
    M = rng.integers(0, K, (B, B))
    if blocky:
        cuts = np.repeat(np.arange(B), rng.integers(1, 10, B))[:B]
        M = M[cuts][:, cuts]
    return np.triu(M) + np.triu(M, 1).T
