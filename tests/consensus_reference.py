"""Plain NumPy restatement of the consensus of M state maps (phylo_hmrf_amd.consensus, csrc/consensus.hip): the definition,
and the yardstick of the GPU call.

  - votes: the one-hot planes of the renumbered maps, summed over the maps: votes[k, v];
  - consensus: np.argmax(votes, axis=0), the LOWEST of the most voted states; support: the votes it got;
  - core: the consensus where support >= min_support, else K;
  - support_hist [K, M + 1], agree [M, K, K], pair [M, M]: np.bincount of index arrays over the stored nodes;
  - bands: per band of d = |dist0 + j - i| (0: d == 0; t >= 1: 2^(t-1) <= d < 2^t), from the full coordinate arrays of the
    stored nodes, the nodes, those with support >= min_support and those with support == M.
"""
import numpy as np

from tests.compare_reference import BANDS, band_of, node_coords

NOT_A_STATE = 255


def renumbered(maps, renumber=None):
    """-> int64 [M, n]: raw state l of map m is renumber[m][l]"""
    maps = np.stack([np.asarray(m, dtype=np.int64).reshape(-1) for m in maps])
    if renumber is None:
        return maps
    ren = np.asarray(renumber, dtype=np.int64)
    return np.stack([ren[m][maps[m]] for m in range(maps.shape[0])])


def vote(maps, K, renumber=None):
    """-> (consensus int64 [n], support int64 [n], the renumbered maps [M, n])"""
    S = renumbered(maps, renumber)
    assert S.min() >= 0 and S.max() < K, "a state is not one of the K (or not a state of its map)"
    votes = (S[:, None, :] == np.arange(K)[None, :, None]).sum(axis=0)          # [K, n]
    cons = np.argmax(votes, axis=0)
    return cons, votes[cons, np.arange(S.shape[1])], S


def tables(cons, support, S, K):
    """-> (support_hist [K, M + 1], agree [M, K, K], pair [M, M])"""
    M, n = S.shape
    hist = np.bincount(cons * (M + 1) + support, minlength=K * (M + 1)).reshape(K, M + 1)
    agree = np.stack([np.bincount(cons * K + S[m], minlength=K * K).reshape(K, K) for m in range(M)])
    pair = np.array([[int((S[a] == S[b]).sum()) for b in range(M)] for a in range(M)], dtype=np.int64).reshape(M, M)
    return hist, agree, pair


def bands(support, M, min_support, H, W, diagonal, dist0):
    ii, jj = node_coords(H, W, diagonal)
    t = band_of(np.abs(dist0 + jj.astype(np.int64) - ii))
    out = np.zeros((BANDS, 3), dtype=np.int64)
    out[:, 0] = np.bincount(t, minlength=BANDS)
    out[:, 1] = np.bincount(t[support >= min_support], minlength=BANDS)
    out[:, 2] = np.bincount(t[support == M], minlength=BANDS)
    return out


def consensus_region(maps, K, H, W, diagonal, dist0=0, min_support=None, renumber=None):
    """-> dict(consensus, support, core uint8 [n]; support_hist, agree, pair, bands int64) of one region"""
    cons, support, S = vote(maps, K, renumber)
    M = S.shape[0]
    assert S.shape[1] == (H * (H + 1) // 2 if diagonal else H * W)
    ms = M // 2 + 1 if min_support is None else min_support
    hist, agree, pair = tables(cons, support, S, K)
    return dict(consensus=cons.astype(np.uint8), support=support.astype(np.uint8),
                core=np.where(support >= ms, cons, K).astype(np.uint8), support_hist=hist, agree=agree, pair=pair,
                bands=bands(support, M, ms, H, W, diagonal, dist0))


def consensus_state_vec(maps, len_vec, K, min_support=None, renumber=None):
    """Region by region -> the dict of phylo_hmrf_amd.consensus.consensus_states (without the scores of the maps)"""
    maps = [np.asarray(m).reshape(-1) for m in maps]
    M, n = len(maps), maps[0].size
    ms = M // 2 + 1 if min_support is None else min_support
    L = np.atleast_2d(np.asarray(len_vec))
    parts = [consensus_region([m[int(row[1]):int(row[2])] for m in maps], K, int(row[3]), int(row[4]), int(row[8]) == 1,
                              int(row[6]) - int(row[5]), ms, renumber) for row in L]
    cat = lambda k: np.concatenate([p[k] for p in parts])
    total = lambda k: np.sum([p[k] for p in parts], axis=0)
    support = cat("support")
    if renumber is None:
        renumber = np.full((M, 64), NOT_A_STATE, dtype=np.uint8)
        renumber[:, :K] = np.arange(K)
    return dict(state_vec=cat("consensus"), support=support, conf=support.astype(np.float32) / np.float32(M),
                core_vec=cat("core") if K < 64 else None, renumber=np.asarray(renumber, dtype=np.uint8),
                support_hist=total("support_hist"), support_hist_region=np.stack([p["support_hist"] for p in parts]),
                agree=total("agree"), pair=total("pair"), pair_agreement=total("pair") / float(n),
                band_counts=np.stack([p["bands"] for p in parts]), K=K, M=M, min_support=ms)
