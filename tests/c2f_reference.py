"""TEST INFRASTRUCTURE ONLY -- float64 reference of the coarse-to-fine start's child problem (phylo_hmrf_amd/csrc/c2f.hip).

A labelling that is constant on the s x s super-cells of a grid block (super-cell of node (i, j) = (i // s, j // s), no offset)
has the energy of a Potts labelling of the coarse grid whose unary terms are the sums over each super-cell's nodes and whose
pair weights are the sums of the fine weights that cross between two super-cells.  From the edge list alone:

  c2f_problem  -> the child's ELL rows (neighbours that exist, in the order NW N NE W E SW S SE, compacted, -1 / 0.0 padded)
                  and its log-probabilities
  coarse_edges -> the child's ELL rows as an edge list, for ref_numpy.mrf_energy
"""
import numpy as np

# the child's adjacency order: (dI, dJ) of its eight neighbours
DIRECTIONS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def fine_coords(H, W, diagonal):
    if diagonal:
        ii, jj = np.triu_indices(H)
    else:
        ii, jj = np.divmod(np.arange(H * W), W)
    return ii.astype(np.int64), jj.astype(np.int64)


def coarse_ids(Hc, Wc, diagonal):
    """idmap[I, J] = node of super-cell (I, J), -1 where there is none (below the diagonal of an upper-triangular block)"""
    if diagonal:
        idmap = -np.ones((Hc, Wc), dtype=np.int64)
        I, J = np.triu_indices(Hc)
        idmap[I, J] = np.arange(I.shape[0])
    else:
        idmap = np.arange(Hc * Wc, dtype=np.int64).reshape(Hc, Wc)
    return idmap


def c2f_problem(eid, w, logprob, H, W, diagonal, s=4, directions=DIRECTIONS):
    """-> (Hc, Wc, cnode[n] super-cell of every node, nbr[nc, 8] int64, wgt[nc, 8] float64, logprob_c[nc, K] float64).
    `directions`: the order of the eight neighbours in a row (tests of the tests pass a wrong one)."""
    eid = np.asarray(eid, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    logprob = np.asarray(logprob, dtype=np.float64)
    ii, jj = fine_coords(H, W, diagonal)
    Hc, Wc = -(-H // s), -(-W // s)
    idmap = coarse_ids(Hc, Wc, diagonal)
    nc = int(idmap.max()) + 1
    I, J = ii // s, jj // s
    cnode = idmap[I, J]
    assert cnode.min() >= 0
    slot_of = dict((d, q) for q, d in enumerate(directions))
    w8 = np.zeros((nc, 8))
    a, b = eid[:, 0], eid[:, 1]
    for src, dst in ((a, b), (b, a)):
        dI, dJ = I[dst] - I[src], J[dst] - J[src]
        assert np.abs(dI).max() <= 1 and np.abs(dJ).max() <= 1       # an edge of the 8-neighbour stencil
        for (di, dj), q in slot_of.items():
            m = (dI == di) & (dJ == dj)
            np.add.at(w8, (cnode[src[m]], np.full(int(m.sum()), q)), w[m])
    nbr = -np.ones((nc, 8), dtype=np.int64)
    wgt = np.zeros((nc, 8))
    cI, cJ = np.nonzero(idmap >= 0)                                 # (row-major: the order of the node ids)
    cnt = np.zeros(nc, dtype=np.int64)
    for q, (di, dj) in enumerate(directions):
        I2, J2 = cI + di, cJ + dj
        ok = (I2 >= 0) & (I2 < Hc) & (J2 >= 0) & (J2 < Wc)
        ok[ok] &= idmap[I2[ok], J2[ok]] >= 0
        rows = np.flatnonzero(ok)
        nbr[rows, cnt[rows]] = idmap[I2[rows], J2[rows]]
        wgt[rows, cnt[rows]] = w8[rows, q]
        cnt[rows] += 1
    K = logprob.shape[1]
    lpc = np.zeros((nc, K))
    np.add.at(lpc, cnode, logprob)
    return Hc, Wc, cnode, nbr, wgt, lpc


def coarse_edges(nbr, wgt):
    """the ELL rows as an edge list -> (eid[E, 2] with id1 < id2, w[E]): every pair once, from its lower end's row"""
    nbr = np.asarray(nbr, dtype=np.int64)
    rows = np.repeat(np.arange(nbr.shape[0]), nbr.shape[1]).reshape(nbr.shape)
    m = nbr > rows
    return np.stack([rows[m], nbr[m]], 1), np.asarray(wgt, dtype=np.float64)[m]


# the shapes of the start kernels' tests: (46, 46) upper triangle -- n = 1081, ragged last super-cell --, ragged rows, exactly the
# thresholds n = 1024 and H = 8, one column / three rows and one row / one column over a multiple of 4
SHAPES = [(46, 46, True), (9, 130, False), (8, 128, False), (32, 33, False), (47, 45, False)]
KS = [1, 2, 7]


def dyadic_inputs(seed, H, W, K, diagonal):
    """a complete 8-neighbour grid with weights in eighths and log-probabilities in halves: every sum is exact in f32
    -> (n, eid, w, logprob)"""
    from oracle import ref_numpy as R
    rng = np.random.default_rng(seed)
    n = H * (H + 1) // 2 if diagonal else H * W
    e = R.grid_edges(np.ones((n, 2)), H, W, diagonal, 8)
    eid = np.int64(e[:, :2])
    w = rng.integers(1, 9, len(eid)) / 8.0
    lp = -rng.integers(0, 12, (n, K)).astype(np.float64) * 0.5
    return n, eid, w, lp
