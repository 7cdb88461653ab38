"""Plain NumPy / SciPy restatement of the reference's small-region smoothing (processing/small_region_test.m with
query_neighbor_state_test.m), on the FULL matrix of a region -- the yardstick of phylo_hmrf_amd.smooth, which works on
the stored upper triangle instead.

One pass, as the scripts run it: components and votes are computed on the map as it is at the start of the pass (mtx1),
every change is written to a copy (mtx1_copy) that becomes the map of the next pass.
  - components: 8-connected components of equal state on the full matrix (bwconncomp's default), area = pixel count;
  - a component is small when its area is <= max_area;
  - a small component of state s collects, with multiplicity, every state != s in the (2h+1) x (2h+1) window around each
    of its pixels whose whole window lies inside the matrix, h = window // 2 (= MATLAB's round((window - 1) / 2));
  - the most frequent collected state k (the lowest on ties, MATLAB's mode) replaces s when count(k) > 0.5 * collected.
Off-diagonal blocks use each pixel's true (row, column) (the script's index arithmetic is only right for square maps).
"""
import numpy as np
from scipy import ndimage


def full_matrix(states, H, W, diagonal):
    """The region's label map as color_map_sub.m builds it: a diagonal block's upper triangle (row-major node order) is
    mirrored into the full symmetric H x H matrix; an off-diagonal block is its H x W matrix in row-major node order."""
    states = np.asarray(states)
    if diagonal:
        assert H == W
        M = np.zeros((H, H), dtype=np.int64)
        ii, jj = np.triu_indices(H)
        M[ii, jj] = states
        M[jj, ii] = states
        return M
    return states.reshape(H, W).astype(np.int64)


def upper_nodes(M, diagonal):
    if diagonal:
        ii, jj = np.triu_indices(M.shape[0])
        return M[ii, jj]
    return M.reshape(-1)


def smooth_pass(M, window, max_area, ratio=0.5):
    """One Jacobi pass on the full matrix M (int).  -> (new matrix, number of small components, number relabelled)."""
    n, m = M.shape
    h = int(window) // 2
    comp = np.zeros((n, m), dtype=np.int64)       # global component id, 0 = none
    comp_state = [0]
    nc_total = 0
    structure = np.ones((3, 3), dtype=bool)
    for s in np.unique(M):
        lab, nc = ndimage.label(M == s, structure=structure)
        sel = lab > 0
        comp[sel] = lab[sel] + nc_total
        comp_state += [int(s)] * nc
        nc_total += nc
    comp_state = np.asarray(comp_state, dtype=np.int64)
    area = np.bincount(comp.reshape(-1), minlength=nc_total + 1)
    small = area <= max_area
    small[0] = False
    K = int(M.max()) + 1
    votes = np.zeros((nc_total + 1) * K, dtype=np.int64)
    if n >= 2 * h + 1 and m >= 2 * h + 1:
        centre = comp[h:n - h, h:m - h]                                # pixels whose whole window lies inside
        cs = small[centre]
        cid = centre[cs]
        cstate = comp_state[cid]
        rows, cols = np.nonzero(cs)
        for dr in range(-h, h + 1):
            for dc in range(-h, h + 1):
                q = M[rows + h + dr, cols + h + dc]
                keep = q != cstate
                votes += np.bincount(cid[keep] * K + q[keep], minlength=votes.shape[0])
    votes = votes.reshape(nc_total + 1, K)
    total = votes.sum(axis=1)
    k = np.argmax(votes, axis=1)                                       # the lowest state on ties, as MATLAB's mode
    best = votes[np.arange(nc_total + 1), k]
    change = small & (total > 0) & (best > ratio * total)
    new_state = np.where(change, k, comp_state)
    out = M.copy()
    hit = change[comp]
    out[hit] = new_state[comp[hit]]
    return out, int(small.sum()), int(change.sum())


def default_max_area(H):
    """read_state_test.m: 80, or 25 for a region less than 100 bins high"""
    return 25 if H < 100 else 80


def smooth_region(states, H, W, diagonal, window=5, max_area=None, n_iter=1):
    """-> the region's smoothed states in node order (same dtype)."""
    states = np.asarray(states)
    if max_area is None:
        max_area = default_max_area(H)
    M = full_matrix(states, H, W, diagonal)
    for _ in range(int(n_iter)):
        M, _, _ = smooth_pass(M, window, max_area)
    return upper_nodes(M, diagonal).astype(states.dtype)


def smooth_state_vec(state_vec, len_vec, window=5, max_area=None, n_iter=1):
    state_vec = np.asarray(state_vec).reshape(-1)
    out = state_vec.copy()
    for row in np.atleast_2d(np.asarray(len_vec)):
        a, b, H, W, diag = int(row[1]), int(row[2]), int(row[3]), int(row[4]), int(row[8]) == 1
        out[a:b] = smooth_region(state_vec[a:b], H, W, diag, window, max_area, n_iter)
    return out
