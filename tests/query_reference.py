"""Host-only restatement of the interval-pair query (phmrf_rect_states, phylo_hmrf_amd.query) as its definitions read; it
shares no code with phylo_hmrf_amd/query.py.  `table` loops over rectangles and cells on the full-matrix index arrays,
`state_query` follows the SET definition: it loops over every stored node of every region and asks whether its bin pair
belongs to the query -- no rectangles, no inclusion-exclusion."""
import numpy as np

CONF_ONE = 1 << 24


def node_cells(H, W, diag):
    """-> (I, J): the row and the column of every stored node in storage order"""
    if diag:
        I, J = np.triu_indices(H)
    else:
        I, J = np.divmod(np.arange(H * W), W)
    return I.astype(np.int64), J.astype(np.int64)


def fixed(conf):
    """-> int64: (uint64)(conf 2^24) per node, the float32 product as the device forms it (exact for a float32 in [0, 1])"""
    c = np.asarray(conf, dtype=np.float32)
    return (c * np.float32(CONF_ONE)).astype(np.int64)


def table(labels, conf, H, W, diag, K, rect, slot, minus, Q):
    """-> (counts int64 [Q, K], conf_sum int64 [Q] or None): rectangle t = (i0, i1, j0, j1) adds (minus[t]: subtracts) its
    stored nodes to row slot[t] (None: t)"""
    labels = np.asarray(labels).astype(np.int64)
    I, J = node_cells(H, W, diag)
    node = -np.ones((H, W), dtype=np.int64)
    node[I, J] = np.arange(I.shape[0])
    counts = np.zeros((Q, K), dtype=np.int64)
    sums = None if conf is None else np.zeros(Q, dtype=np.int64)
    f = None if conf is None else fixed(conf)
    for t, (i0, i1, j0, j1) in enumerate(np.asarray(rect, dtype=np.int64).reshape(-1, 4)):
        q = t if slot is None else int(slot[t])
        sign = -1 if (minus is not None and minus[t]) else 1
        cells = node[max(i0, 0):max(min(i1, H), 0), max(j0, 0):max(min(j1, W), 0)]     # the rectangle on the full matrix
        v = cells[cells >= 0]                                                         # ... and its stored nodes
        np.add.at(counts[q], labels[v], sign)
        if sums is not None:
            sums[q] += sign * int(f[v].sum())
    return counts, sums


def state_query(state_vec, len_vec, queries, K, conf=None):
    """-> (counts int64 [Q, K], conf_sum int64 [Q] or None) by the set definition: a stored node (i, j) of a region of the
    query's chromosome stands for the bin pair {x, y} = {start_bin1 + i, start_bin2 + j}; it belongs to the query when
    (x in A and y in B) or (x in B and y in A)"""
    s = np.asarray(state_vec).astype(np.int64).reshape(-1)
    queries = np.asarray(queries, dtype=np.int64).reshape(-1, 5)
    counts = np.zeros((queries.shape[0], K), dtype=np.int64)
    sums = None if conf is None else np.zeros(queries.shape[0], dtype=np.int64)
    f = None if conf is None else fixed(conf)
    for row in np.asarray(len_vec, dtype=np.int64):
        lo, hi, H, W, s1, s2, diag, chrom = (int(row[c]) for c in (1, 2, 3, 4, 5, 6, 8, 9))
        I, J = node_cells(H, W, diag)
        x, y = I + s1, J + s2
        lab = s[lo:hi]
        for t, (c, a0, a1, b0, b1) in enumerate(queries):
            if c != chrom:
                continue
            xa, xb, ya, yb = (a0 <= x) & (x < a1), (b0 <= x) & (x < b1), (a0 <= y) & (y < a1), (b0 <= y) & (y < b1)
            inside = (xa & yb) | (xb & ya)
            counts[t] += np.bincount(lab[inside], minlength=K)
            if sums is not None:
                sums[t] += int(f[lo:hi][inside].sum())
    return counts, sums


def pairs_of(a0, a1, b0, b1):
    """-> the number of bin pairs of a query, by listing the set"""
    A, B = range(a0, a1), range(b0, b1)
    return len({(min(i, j), max(i, j)) for i in A for j in B})
