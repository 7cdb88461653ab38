"""Float64 NumPy reference of the energy family (csrc/kernels.hip: energy_kernel, energy_grid_kernel, energy_delta_grid_kernel,
energy_diff_grid_kernel), from an edge list.  No GPU, no library call.

    E(l) = sum_i un[i, l_i]  +  beta * sum_{(a, b) in edges} w_ab [l_a != l_b]

Every function returns the two sums apart, the pair sum WITHOUT beta (the caller multiplies: the library's entry points
report beta x pair).

Owned rows.  A row tile counts the grid rows [r0, r1) it owns: the unary terms of the nodes on those rows, and the edges
that BELONG to those rows.  An edge belongs to its upper / left end -- in the row-major node order of a rectangular and of
an upper-triangular block that is the end with the smaller node id: E, SW, S and SE edges of a node are its own, W, NW, N
and NE edges are the other end's.  So the edges between a tile's last owned row and the halo row below it are the tile's,
the edges between its upper halo row and its first owned row are the upper neighbour's, and edges inside a halo row are
nobody's here.  Summed over the tiles of a block every node and every edge is counted exactly once.

The lattice (tests/test_gpu_estep._integer_problem): unaries are multiples of 0.5, weights multiples of 1/8, beta is one of
BETAS.  Every term, every f32 sum of a node's four forward weights (<= 4), every f64 sum over a block (< 2^53 eighths) and
the 2^-20 fixed point of deterministic mode hold such numbers exactly, whatever the order of summation: the device's sums
must EQUAL this reference, and the tests that use it assert equality."""
import numpy as np

from oracle import ref_numpy as R

BETAS = (0.5, 1.0, 2.0)


# ---- geometry -----------------------------------------------------------------------------------------------------------
def node_count(H, W, diagonal):
    return H * (H + 1) // 2 if diagonal else H * W


def grid_rows_cols(H, W, diagonal):
    """grid (row, column) of every node, in node order (upper-triangular blocks: row-major over the cells with j >= i)"""
    if diagonal:
        ii, jj = np.triu_indices(H)
    else:
        ii, jj = np.divmod(np.arange(H * W), W)
    return ii.astype(np.int64), jj.astype(np.int64)


def stencil(H, W, diagonal, num_neighbor):
    """the complete stencil's edge list [E, 2], id1 < id2"""
    n = node_count(H, W, diagonal)
    e = R.grid_edges(np.ones((n, 1)), H, W, diagonal, num_neighbor)
    eid = np.int64(e[:, :2]).reshape(-1, 2)
    return np.stack([eid.min(axis=1), eid.max(axis=1)], 1) if len(eid) else np.zeros((0, 2), dtype=np.int64)


def lattice_problem(seed, H, W, K, diagonal, num_neighbor=8):
    """-> n, eid[E, 2], w[E] (eighths in [1/8, 1]), un[n, K] (halves in [-2, 5.5]; unary = -logprob)"""
    rng = np.random.default_rng(seed)
    n = node_count(H, W, diagonal)
    eid = stencil(H, W, diagonal, num_neighbor)
    w = rng.integers(1, 9, len(eid)) / 8.0
    un = rng.integers(0, 12, (n, K)).astype(np.float64) * 0.5
    un[np.arange(n), rng.integers(0, K, n)] -= 2.0
    return n, eid, w, un


def is_lattice(w, un, beta):
    return bool(np.array_equal(w * 8, np.round(w * 8)) and np.array_equal(un * 2, np.round(un * 2)) and beta in BETAS)


# ---- the energy -----------------------------------------------------------------------------------------------------------
def _owner(eid):
    return np.minimum(eid[:, 0], eid[:, 1])         # the upper / left end


def _row_mask(n, node_row, rows):
    if rows is None:
        return np.ones(n, dtype=bool)
    node_row = np.asarray(node_row)
    return (node_row >= rows[0]) & (node_row < rows[1])


def energy(eid, w, un, labels, node_row=None, rows=None):
    """(unary, pair) of a labelling; rows = (r0, r1): over the owned rows only (node_row[i] = grid row of node i)"""
    l = np.asarray(labels, dtype=np.int64)
    n = l.shape[0]
    own = _row_mask(n, node_row, rows)
    eu = float(np.sum(un[np.arange(n), l][own]))
    cut = l[eid[:, 0]] != l[eid[:, 1]]
    ep = float(np.sum((np.asarray(w, dtype=np.float64) * cut)[own[_owner(eid)]]))
    return eu, ep


def energy_difference(eid, w, un, a, b, node_row=None, rows=None):
    """E(a) - E(b) two ways -> ((unary, pair) as the difference of two energies, (unary, pair) from the differing nodes).
    The second is the kernels' argument: a node's unary term differs only where its label does, and an edge's term only
    where an end's label does -- the unary terms of the differing nodes and the edges with a differing end, each edge at its
    owner, are the whole difference."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    n = a.shape[0]
    ua, pa = energy(eid, w, un, a, node_row, rows)
    ub, pb = energy(eid, w, un, b, node_row, rows)
    own = _row_mask(n, node_row, rows)
    differs = a != b
    idx = np.flatnonzero(differs & own)
    du = float(np.sum(un[idx, a[idx]] - un[idx, b[idx]]))
    touched = (differs[eid[:, 0]] | differs[eid[:, 1]]) & own[_owner(eid)]
    e = eid[touched]
    term = (a[e[:, 0]] != a[e[:, 1]]).astype(np.float64) - (b[e[:, 0]] != b[e[:, 1]]).astype(np.float64)
    dp = float(np.sum(np.asarray(w, dtype=np.float64)[touched] * term))
    return (ua - ub, pa - pb), (du, dp)


def tile_sums(eid, w, un, labels, node_row, row_ranges):
    """[(unary, pair)] over the owned rows [r0, r1) of every tile, all on the one labelling of the whole block"""
    return [energy(eid, w, un, labels, node_row, rr) for rr in row_ranges]


def adjacency_energy(eid, w, un, labels):
    """the adjacency form (energy_kernel): half the sum over every node's neighbours -> (unary, pair)"""
    l = np.asarray(labels, dtype=np.int64)
    n = l.shape[0]
    src = np.concatenate([eid[:, 0], eid[:, 1]])
    dst = np.concatenate([eid[:, 1], eid[:, 0]])
    ww = np.concatenate([w, w]).astype(np.float64)
    per_node = np.bincount(src, weights=ww * (l[src] != l[dst]), minlength=n)
    return float(np.sum(un[np.arange(n), l])), 0.5 * float(np.sum(per_node))


# ---- a row tile's own problem -----------------------------------------------------------------------------------------------
def tile_local(eid, w, un, H, W, diagonal, s0, s1):
    """The stored rows [s0, s1) of a block as a problem of their own (what a tile holds): -> node0, eid_local, w_local,
    un_local, node_row_local (0 = the first stored row).  Edges with an end outside the stored rows are dropped."""
    ii, _ = grid_rows_cols(H, W, diagonal)
    keep_n = np.flatnonzero((ii >= s0) & (ii < s1))
    node0, n_loc = int(keep_n[0]), len(keep_n)
    assert np.array_equal(keep_n, np.arange(node0, node0 + n_loc))          # (rows are contiguous in node order)
    keep_e = (eid.min(axis=1) >= node0) & (eid.max(axis=1) < node0 + n_loc)
    return node0, eid[keep_e] - node0, np.asarray(w)[keep_e], un[node0:node0 + n_loc], ii[keep_n] - s0


# ---- labellings -------------------------------------------------------------------------------------------------------------
def labelling(kind, rng, H, W, diagonal, K):
    """constant | random | checkerboard (every edge of the 4-stencil cut, and with K >= 4 every edge of the 8-stencil) |
    absent (random without label K - 1; K = 1: constant)"""
    ii, jj = grid_rows_cols(H, W, diagonal)
    n = ii.shape[0]
    if kind == "constant":
        return np.full(n, min(1, K - 1), dtype=np.int64)
    if kind == "random":
        return rng.integers(0, K, n)
    if kind == "checkerboard":
        return ((ii % 2) * 2 + (jj % 2)) % K if K >= 4 else (ii + jj) % K
    assert kind == "absent"
    return rng.integers(0, max(K - 1, 1), n)
