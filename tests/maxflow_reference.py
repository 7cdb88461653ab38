"""TEST INFRASTRUCTURE ONLY -- what one alpha-expansion of a general graph (csrc/maxflow.hip) has to return, by an exact
integer max-flow on the host (SciPy / NetworkX; no device code, nothing of gco).

The binary problem (header of maxflow.hip).  x_i = 1: node i takes alpha; active = the nodes with l_i != alpha.
  E(x) - E(0) = sum_i theta_i x_i + sum_{arcs i->j} c_ij x_i (1 - x_j)
  theta_i = lp[i, l_i] - lp[i, alpha] - beta sum_{j: l_j = alpha} w_ij - beta/2 sum_{j active, l_j != l_i} w_ij
  c_ij = c_ji = beta w_ij (1 - [l_i != l_j] / 2)                          (i, j active)
theta_i < 0 is a source arc of capacity -theta_i, theta_i > 0 a sink arc; a minimum s-t cut is a minimum of E.

quantised_problem   the INTEGER problem the device solves: float64 arithmetic on inputs rounded to float32, the largest
                    single term (`top`) at 2^24, pair capacities truncated, switch costs rounded up plus one quantum.
                    Where w, lp are dyadic and top is a power of two, every float32 operation of the device is exact and
                    this is the device's problem to the last bit.
kept_side           the active nodes that cannot reach the sink in the residual graph of a maximum flow of that problem.
                    That set is the same for EVERY maximum flow (it is the largest source side among the minimum cuts), so
                    it does not depend on the algorithm or its schedule: the device's expansion must switch exactly it.
exact_expansion_energy   the true optimum of the unquantised problem (float64 inputs, top at 2^40, Python integers).
expansion_allowance how far above that optimum a correct device expansion may end, derived term by term.

Pure host code: tests/test_maxflow_reference.py checks all of it against brute force without a GPU."""
import math

import numpy as np

from oracle import ref_numpy as R

U32 = 2.0 ** -24          # the largest relative error of one float32 rounding (half an ulp)


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _terms(n, edges, w, lp, labels, beta, alpha):
    """-> (active[n] bool, theta[n], arcs (i, j) with i < j between two active nodes, their c_ij, the largest beta*w over
    the arcs of active nodes), all float64 from the inputs as given."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    labels = np.asarray(labels, dtype=np.int64)
    act = labels != alpha
    theta = np.where(act, lp[np.arange(n), labels] - lp[:, alpha], 0.0)
    a, b = edges[:, 0], edges[:, 1]
    bw = beta * w
    for u, v in ((a, b), (b, a)):
        to_alpha = act[u] & ~act[v]
        np.subtract.at(theta, u[to_alpha], bw[to_alpha])
        differ = act[u] & act[v] & (labels[u] != labels[v])
        np.subtract.at(theta, u[differ], 0.5 * bw[differ])
    both = act[a] & act[b]
    c = bw[both] * np.where(labels[a[both]] != labels[b[both]], 0.5, 1.0)
    touched = act[a] | act[b]
    wmax = float(bw[touched].max()) if touched.any() else 0.0
    return act, theta, edges[both], c, wmax


def quantised_problem(n, edges, w, lp, labels, beta, alpha):
    """-> dict(n, active, top, scale, arcs[m,2], cap[m] int64 (both directions), cost[n] int64: > 0 a sink arc, < 0 a
    source arc of capacity -cost; 0 on inactive nodes)."""
    lp32, w32, b32 = _f32(lp), _f32(w), float(np.float32(beta))
    act, theta, arcs, c, wmax = _terms(n, edges, w32, lp32, labels, b32, alpha)
    top = max(wmax, float(np.abs(theta).max()) if n else 0.0)
    scale = 2.0 ** 24 / top if top > 0 else 0.0
    cap = np.floor(scale * c).astype(np.int64)
    cost = np.where(act, np.ceil(scale * theta).astype(np.int64) + 1, 0)
    return dict(n=n, active=act, top=top, scale=scale, arcs=arcs, cap=cap, cost=cost, theta=theta)


def is_power_of_two(x):
    return x > 0 and math.frexp(x)[0] == 0.5


def kept_side(problem):
    """the nodes that take alpha: active, and without a residual path to the sink after a maximum flow -> bool[n]"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import breadth_first_order, maximum_flow
    n, arcs, cap, cost = problem["n"], problem["arcs"], problem["cap"], problem["cost"]
    s, t = n, n + 1
    src, snk = np.flatnonzero(cost < 0), np.flatnonzero(cost > 0)
    rows = np.concatenate([arcs[:, 0], arcs[:, 1], np.full(len(src), s), snk])
    cols = np.concatenate([arcs[:, 1], arcs[:, 0], src, np.full(len(snk), t)])
    vals = np.concatenate([cap, cap, -cost[src], cost[snk]])
    assert vals.size == 0 or vals.max() < 2 ** 31
    capm = csr_matrix((vals.astype(np.int32), (rows, cols)), shape=(n + 2, n + 2))
    flow = maximum_flow(capm, s, t).flow
    res = (capm - flow).tocsr()                         # (flow is antisymmetric: this holds the reverse arcs as well)
    res.data = (res.data > 0).astype(np.int8)
    res.eliminate_zeros()
    reach = breadth_first_order(res.T.tocsr(), t, directed=True, return_predecessors=False)
    out = problem["active"].copy()
    out[reach[reach < n]] = False
    return out


def exact_expansion(n, edges, w, lp, labels, beta, alpha, bits=40):
    """The optimum of the unquantised expansion -> (energy float64 by oracle.ref_numpy.mrf_energy, switched bool[n]).
    Integer max-flow with the largest term at 2^bits (capacities rounded to nearest: 2^-bits of top per term)."""
    import networkx as nx
    lp = np.asarray(lp, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    act, theta, arcs, c, wmax = _terms(n, edges, w, lp, labels, float(beta), alpha)
    top = max(wmax, float(np.abs(theta).max()) if n else 0.0)
    switched = np.zeros(n, dtype=bool)
    if top > 0:
        scale = 2.0 ** bits / top
        g = nx.DiGraph()
        g.add_nodes_from(("s", "t"))
        for (i, j), cij in zip(arcs.tolist(), c.tolist()):
            q = int(round(scale * cij))
            if q > 0:
                g.add_edge(i, j, capacity=q)
                g.add_edge(j, i, capacity=q)
        for i in np.flatnonzero(act).tolist():
            q = int(round(scale * theta[i]))
            if q < 0:
                g.add_edge("s", i, capacity=-q)
            elif q > 0:
                g.add_edge(i, "t", capacity=q)
        _, (source_side, _) = nx.minimum_cut(g, "s", "t")
        source_side.discard("s")
        switched[list(source_side)] = True
    cand = labels.copy()
    cand[switched] = alpha
    return R.mrf_energy(cand, lp, edges, np.asarray(w, dtype=np.float64), float(beta))[0], switched


def exact_expansion_energy(n, edges, w, lp, labels, beta, alpha, bits=40):
    return exact_expansion(n, edges, w, lp, labels, beta, alpha, bits)[0]


def expansion_allowance(n, edges, w, lp, labels, beta, alpha, got, best):
    """How far e(got) may lie above e(best), for the set `got` that a correct device expansion switches and ANY other set
    `best` (the exact optimum; the empty set for "the energy does not rise"), in energy units.

    `got` minimises the quantised cost Q, so with F the true cost and s the scale
      F(got) - F(best) <= [F(got) - Q(got) / s] + [Q(best) / s - F(best)].
    A node in both sets and an arc cut by both cancel in the two brackets; what is left, with q = top / 2^24 (one quantum,
    `top` the device's own: the largest single term) and u = 2^-24 (one float32 rounding, relative):

      a node only in `got`    r_i                  its quantised cost is rounded UP: only float32 rounding can undercount it
      a node only in `best`   2 q + r_i            ceil(.) < 1 quantum, and the "+1" of the tie rule
      an arc cut by `got` only    q + 4 u c_ij     the truncation of its capacity; w stored in float32, scale = 2^24 / top,
                                                   scale * beta, (.) * w: one rounding each (x 0.5 is exact)
      an arc cut by `best` only   4 u c_ij

      r_i = u (|lp_i,alpha| + |lp_i,l| + (t_i + 1) P_i + 2 beta sum'_j w_ij + 2 |theta_i|)
        lp stored in float32 (two roundings); theta_i summed in float32 from lp_i,l - lp_i,alpha downwards over the t_i
        neighbours that contribute (label alpha, or another label than l_i): t_i + 1 roundings of a partial sum that lies
        between its first and its last value, P_i = max(|lp_i,l - lp_i,alpha|, |theta_i|), in ANY order; each such w_ij stored
        in float32 and multiplied by beta; scale and scale * theta_i rounded (u relative each).
    A fused multiply-add only removes roundings.  The float64 scoring of the two labellings adds 1e-13 of |e| (n + E terms).
    Not multiplied by n, and not by the sum of all weights."""
    lp = np.asarray(lp, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    got, best = np.asarray(got, dtype=bool), np.asarray(best, dtype=bool)
    p = quantised_problem(n, edges, w, lp, labels, beta, alpha)
    q = p["top"] * U32
    a, b = edges[:, 0], edges[:, 1]
    act = labels != alpha
    contributes = (labels[a] != labels[b])                       # (for an active node: the neighbour is alpha or differs)
    t = np.bincount(a, weights=contributes, minlength=n) + np.bincount(b, weights=contributes, minlength=n)
    ws = np.bincount(a, weights=w * contributes, minlength=n) + np.bincount(b, weights=w * contributes, minlength=n)
    idx = np.arange(n)
    first = np.abs(lp[idx, labels] - lp[:, alpha])
    r = U32 * (np.abs(lp[:, alpha]) + np.abs(lp[idx, labels]) + (t + 1) * np.maximum(first, np.abs(p["theta"]))
               + 2 * beta * ws + 2 * np.abs(p["theta"]))
    both = act[a] & act[b]
    c = beta * w * np.where(labels[a] != labels[b], 0.5, 1.0)
    cut_got, cut_best = both & (got[a] != got[b]), both & (best[a] != best[b])
    e0 = abs(R.mrf_energy(labels, lp, edges, w, float(beta))[0])
    return float(r[got & ~best].sum() + (2 * q + r[best & ~got]).sum()
                 + (q + 4 * U32 * c[cut_got & ~cut_best]).sum() + 4 * U32 * c[cut_best & ~cut_got].sum() + 1e-13 * e0)


def brute_force(n, edges, w, lp, labels, beta, alpha):
    """all 2^active switch sets -> (kept_side by the quantised cost, ties to the LARGEST set; the least float64 energy)."""
    import itertools
    labels = np.asarray(labels, dtype=np.int64)
    lp = np.asarray(lp, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    p = quantised_problem(n, edges, w, lp, labels, beta, alpha)
    active = np.flatnonzero(p["active"])
    assert len(active) <= 16
    best_q, best_set, best_e = None, None, np.inf
    for bits in itertools.product((False, True), repeat=len(active)):
        sw = np.zeros(n, dtype=bool)
        sw[active] = bits
        cut = sw[p["arcs"][:, 0]] != sw[p["arcs"][:, 1]]
        cost = int(p["cost"][sw].sum() + p["cap"][cut].sum())
        key = (cost, -int(sw.sum()))
        if best_q is None or key < best_q:
            best_q, best_set = key, sw
        cand = labels.copy()
        cand[sw] = alpha
        best_e = min(best_e, R.mrf_energy(cand, lp, edges, np.asarray(w, dtype=np.float64), float(beta))[0])
    return best_set, best_e


# ---- the problems of tests/test_gpu_maxflow.py (built here so that the CPU tests check the recipe as well) -------------
def dyadic_problem(rng, n, pairs, K, beta, wmax=4.0, lpmax=4.0):
    """w, lp multiples of 1/64 below wmax / lpmax on the given pairs -> (edges, w, lp, labels)"""
    edges = np.asarray(sorted(set((min(i, j), max(i, j)) for i, j in pairs)), dtype=np.int64).reshape(-1, 2)
    w = rng.integers(1, int(wmax * 64), len(edges)) / 64.0
    lp = -rng.integers(0, int(lpmax * 64), (n, K)) / 64.0
    return edges, w, lp, rng.integers(0, K, n)


def with_anchor(n, edges, w, lp, labels, beta, alpha):
    """Two more nodes of equal label (not alpha), one edge of weight 128 / beta between them, zero unaries: the largest
    single term is then 128 exactly, provided every other term is below it -> (n + 2, edges, w, lp, labels)."""
    K = lp.shape[1]
    edges = np.concatenate([np.asarray(edges, dtype=np.int64).reshape(-1, 2), [[n, n + 1]]])
    w = np.concatenate([w, [128.0 / beta]])
    lp = np.concatenate([lp, np.zeros((2, K))])
    labels = np.concatenate([labels, [(alpha + 1) % K] * 2])
    return n + 2, edges, w, lp, labels


def sparse_pairs(rng, n):
    """a spanning path plus every other pair with probability 3 / n"""
    m = rng.poisson(1.5 * n)
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    return [(k, k + 1) for k in range(n - 1)] + [(int(a), int(b)) for a, b in zip(i, j) if a != b]


def far_sink_path(n, K=3, alpha=1):
    """Point 1: a path of n active nodes, every one a mild source (theta = -1/64) but the last, which is the only sink
    and the largest term (theta = +128): nothing may switch, and the first node sits at BFS level n."""
    edges = np.array([(i, i + 1) for i in range(n - 1)], dtype=np.int64).reshape(-1, 2)
    w = np.full(n - 1, 32.0)                      # (capacity 2^22 at beta = 1: all n sources together stay below it)
    labels = np.zeros(n, dtype=np.int64)
    lp = np.zeros((n, K))
    lp[:, alpha] = 1.0 / 64                       # theta = lp[l] - lp[alpha] = -1/64
    lp[n - 1, alpha] = -128.0
    return edges, w, lp, labels


def deep_path(n, K=3, alpha=1):
    """Point 2: node 1 is a strong source (excess 96 over arcs of capacity 32 beta), node n-1 the only large sink (+128), the
    nodes between are slightly negative (-1/64: they drain nothing).  The flow saturates the path, so a prefix switches."""
    edges, w, lp, labels = far_sink_path(n, K, alpha)
    lp[1, alpha] = 96.0
    return edges, w, lp, labels
