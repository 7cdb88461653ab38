"""TEST INFRASTRUCTURE ONLY -- seeded cases for the move kernels OFF the complete stencil grid: graphs that are no grid
(the path of pygco_compat.cut_general_graph: greedy colouring, adjacency-row component kernels, path families) and grid
blocks whose edge list is a SUBSET of the stencil (phmrf_block_set_grid accepts it and records the grid as incomplete).

Pure NumPy / SciPy, no GPU: tests/test_graph_moves_cpu.py checks the builders and that the cases discriminate,
tests/test_gpu_graph_moves.py runs them against the kernels.

Arithmetic.  Every case is an "integer problem": unaries are multiples of 0.5, weights multiples of 1/8 and beta is one
of BETAS, so every term of an energy lies on the 1/16 grid.  check_exact() asserts from the inputs alone that a
whole-graph sum stays below 2^20 sixteenths (f32 sums, f32 atomics in any order and the 2^-16 fixed point of the
deterministic component table are then exact), and check_component_tables() asserts from the MODEL alone that every entry
of every component table the tests will see has magnitude <= 4096: the margin of the component decision,
1e-5 |tc| + 1e-6 <= 0.042, plus one f32 ulp of such a sum stays below the 1/16 by which two gains differ at the least, so
the f32 and the float64 decisions cannot differ.  Hence the kernels must reproduce the float64 move model label for label.
"""
import numpy as np

from oracle import mrf_moves as M
from oracle import ref_numpy as R
from oracle import synth

BETAS = (0.5, 1.0, 2.0)
N_COMPONENT_PASSES = 3
N_ICM_SWEEPS = 3
TABLE_BOUND = 4096.0


class Case(object):
    """name, n, K, beta, eid[E,2] (id1 < id2), w[E], un[n,K] (= -logprob), init[n] (where ICM starts), comp_start[n] (where
    the component passes start), grid = None or (H, W, diagonal, num_neighbor as declared), g = the float64 graph."""

    def __init__(self, name, n, K, beta, eid, w, un, init, grid=None):
        self.name, self.n, self.K, self.beta, self.grid = name, int(n), int(K), float(beta), grid
        self.eid = np.ascontiguousarray(eid, dtype=np.int64).reshape(-1, 2)
        self.w = np.asarray(w, dtype=np.float64)
        self.un = np.asarray(un, dtype=np.float64)
        self.lp = -self.un
        self.init = np.asarray(init, dtype=np.int64)
        self.g = M.Graph(self.n, self.eid, self.w)
        self.comp_start = None
        deg = np.diff(self.g.row_ptr)
        self.max_degree = int(deg.max())
        self.D = max(4, (self.max_degree + 3) // 4 * 4)          # the row width phmrf_block_set_graph chooses

    def __repr__(self):
        return self.name

    def colours(self):
        """the ICM colour classes the library uses for this block -> (colour[n], n_colours)"""
        if self.grid is not None:
            return M.icm_colours(*self.grid[:3])
        return greedy_colouring(self.g)


# ------------------------------------------------------------------------------------------------ shared pieces
def greedy_colouring(g):
    """The host's colouring of a graph without a grid (phmrf_block_set_graph): nodes in index order, each takes the smallest
    colour that none of its already coloured neighbours has -> (colour[n], n_colours)."""
    colour = -np.ones(g.n, dtype=np.int64)
    for i in range(g.n):
        used = set(colour[g.col[g.row_ptr[i]:g.row_ptr[i + 1]]].tolist())
        c = 0
        while c in used:
            c += 1
        colour[i] = c
    return colour, int(colour.max()) + 1


def graph_blobs(rng, g, n_seeds):
    """Connected regions of a graph: breadth-first growth from n_seeds random nodes at once -> region[n] (a node no seed
    reaches is a region of its own)."""
    region = -np.ones(g.n, dtype=np.int64)
    front = rng.choice(g.n, size=min(n_seeds, g.n), replace=False)
    region[front] = np.arange(len(front))
    while len(front):
        nxt = []
        for v in front:
            for u in g.col[g.row_ptr[v]:g.row_ptr[v + 1]]:
                if region[u] < 0:
                    region[u] = region[v]
                    nxt.append(u)
        front = np.asarray(nxt, dtype=np.int64)
    lone = np.flatnonzero(region < 0)
    region[lone] = region.max() + 1 + np.arange(len(lone))
    return region


def integer_terms(rng, n, K, truth, levels=4, bias=1.0):
    """unaries: multiples of 0.5 in [0, levels / 2), the true label `bias` cheaper.  The defaults keep a node's own terms
    below what its equal-label neighbours weigh, so that ICM leaves the inside of a wrongly labelled region alone and the
    region is left for the component pass to move as a whole."""
    un = rng.integers(0, levels, (n, K)).astype(np.float64) * 0.5
    un[np.arange(n), truth] -= bias
    return un


def blobby_start(rng, K, region, truth, noise=0.15):
    """Labels that start blobby plus noise: every other region carries a wrong label as a whole (a component worth moving),
    and a fraction `noise` of the nodes a random one."""
    wrong = (region % 2 == 1)
    lab = np.where(wrong, (truth + 1 + region % max(K - 1, 1)) % K, truth)
    flip = rng.random(len(lab)) < noise
    return np.where(flip, rng.integers(0, K, len(lab)), lab).astype(np.int64)


def finish(case, icm_before_components=True):
    """comp_start: a few model ICM sweeps from init give components worth relabelling (or init itself); then the two
    conditions of the module docstring."""
    lab = case.init.copy()
    if icm_before_components:
        col, nc = case.colours()
        for _ in range(N_ICM_SWEEPS):
            M.icm_sweep(case.g, case.un, lab, case.beta, col, nc)
    case.comp_start = lab
    check_exact(case)
    check_component_tables(case)
    return case


def check_exact(case):
    assert case.beta in BETAS
    assert np.array_equal(case.un * 2, np.round(case.un * 2)) and np.array_equal(case.w * 8, np.round(case.w * 8))
    assert case.init.min() >= 0 and case.init.max() < case.K
    total = float(np.abs(case.un).max(axis=1).sum() + case.beta * case.w.sum())
    assert total * 16 < 2 ** 20, (case.name, total)


def check_component_tables(case):
    """every entry of the model's component table, in every component pass the tests run (from comp_start, and from init
    where a test starts the passes there), has magnitude <= TABLE_BOUND"""
    worst = 0.0
    for start in (case.comp_start, case.init):
        lab = start.copy()
        for _ in range(N_COMPONENT_PASSES):
            U = M.component_table(case.g, case.un, lab, case.beta)[0]
            worst = max(worst, float(np.abs(U).max()))
            M.component_pass(case.g, case.un, lab, case.beta)
    assert worst <= TABLE_BOUND, (case.name, worst)
    case.table_max = worst


def _pairs(a, b):
    """unique undirected pairs without self loops -> eid[E,2], id1 < id2, sorted"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    if len(lo) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    return np.unique(np.stack([lo, hi], 1), axis=0)


def _weights(rng, E):
    return rng.integers(1, 9, E) / 8.0


def _general(name, seed, n, K, beta, eid, n_seeds, levels=4):
    rng = np.random.default_rng(seed)
    w = _weights(rng, len(eid))
    g = M.Graph(n, eid, w)
    region = graph_blobs(rng, g, n_seeds)
    truth = rng.integers(0, K, region.max() + 1)[region]
    un = integer_terms(rng, n, K, truth, levels)
    init = blobby_start(rng, K, region, truth)
    return finish(Case(name, n, K, beta, eid, w, un, init))


# ------------------------------------------------------------------------------------------------ graphs that are no grid
def knn_case(seed, n, k, K, beta):
    """k nearest neighbours of random points (oracle/synth.make_knn_block): ragged degrees, rows wider than 8"""
    eid = np.int64(synth.make_knn_block(seed, n, 4, 3, k=k)["edges"][:, :2])
    return _general("knn-k%d-n%d-K%d" % (k, n, K), seed, n, K, beta, eid, n_seeds=max(2, n // 60))


def sparse_case(seed, n, K, beta):
    """random pairs, mean degree about 3: a giant component, many small ones and nodes of degree 0"""
    rng = np.random.default_rng(seed + 1000)
    m = (3 * n) // 2
    eid = _pairs(rng.integers(0, n, m), rng.integers(0, n, m))
    return _general("sparse-n%d-K%d" % (n, K), seed, n, K, beta, eid, n_seeds=max(2, n // 40))


def hub_case(seed, n, K, beta):
    """a ring and one node of degree 64, the limit of phmrf_block_set_graph: rows of width 64"""
    rng = np.random.default_rng(seed + 2000)
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)
    hub = n // 2 + 1
    others = np.setdiff1d(np.arange(n), [hub - 1, hub, hub + 1])
    spokes = rng.choice(others, size=62, replace=False)
    eid = _pairs(np.concatenate([ring[:, 0], np.full(62, hub)]), np.concatenate([ring[:, 1], spokes]))
    return _general("hub-n%d-K%d" % (n, K), seed, n, K, beta, eid, n_seeds=max(2, n // 25))


def deg4_case(seed, n, K, beta):
    """a ring with chords, no node of degree above 4: rows of width 4, the register path behind a padded load_row"""
    rng = np.random.default_rng(seed + 3000)
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)
    a, b = [], []
    for _ in range(2):                                       # two random matchings: at most two chords per node
        perm = rng.permutation(n)[:(n // 2) * 2 - 2 * (n // 10)]
        a.append(perm[0::2])
        b.append(perm[1::2])
    eid = _pairs(np.concatenate([ring[:, 0]] + a), np.concatenate([ring[:, 1]] + b))
    return _general("deg4-n%d-K%d" % (n, K), seed, n, K, beta, eid, n_seeds=max(2, n // 30))


# run lengths of the path case's initial labels and where they start: at, one before and one after multiples of 64 (a wave
# chunk of cc_init_kernel) and of 256 (its workgroup); "fill" stretches are runs of 1, 2 and 3 nodes
PATH_N = 2500
PATH_RUNS = [(0, 64), (64, 63), (127, 1), (128, 127), (255, 2), (257, 256), (513, 255), (768, 257), (1025, 65),
             (1151, 129), (1280, 128), (1408, 1000)]
PATH_FILL = [(1090, 1151), (2408, 2500)]
PATH_RUN_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
# start residues the layout claims: (modulus, residue) -> starts of PATH_RUNS
PATH_CLAIMS = {(64, 0): (0, 64, 128, 768, 1280, 1408), (64, 63): (127, 255, 1151), (64, 1): (257, 513, 1025),
               (256, 0): (0, 768, 1280), (256, 255): (255,), (256, 1): (257, 513, 1025)}


def path_run_labels(K):
    """the initial labels of the path case -> (labels[PATH_N], starts of all runs, fill runs included)"""
    lab = -np.ones(PATH_N, dtype=np.int64)
    pieces = list(PATH_RUNS)
    for a, b in PATH_FILL:
        p, q = a, 0
        while p < b:
            ln = min((1, 2, 3)[q % 3], b - p)
            pieces.append((p, ln))
            p += ln
            q += 1
    pieces.sort()
    for r, (start, ln) in enumerate(pieces):
        lab[start:start + ln] = r % K
    assert lab.min() >= 0 and sum(ln for _, ln in pieces) == PATH_N
    return lab, np.array([s for s, _ in pieces])


def path_case(seed, K, beta):
    """nodes 0 - 1 - ... - (n - 1) on one path plus random chords; the labels come in the runs of PATH_RUNS, and the
    component passes start from them as they are (an ICM sweep would break the runs up)"""
    n = PATH_N
    rng = np.random.default_rng(seed + 4000)
    m = n // 10
    eid = _pairs(np.concatenate([np.arange(n - 1), rng.integers(0, n, m)]), np.concatenate([np.arange(1, n), rng.integers(0, n, m)]))
    w = _weights(rng, len(eid))
    init, starts = path_run_labels(K)
    run = np.searchsorted(starts, np.arange(n), side="right") - 1
    # a third of the runs would rather carry another label as a whole
    truth = np.where(run % 3 == 1, (init + 1) % K, init)
    un = integer_terms(rng, n, K, truth)
    return finish(Case("path-n%d-K%d" % (n, K), n, K, beta, eid, w, un, init), icm_before_components=False)


def tiny_case(n, K, beta):
    rng = np.random.default_rng(n)
    eid = np.stack([np.arange(n - 1), np.arange(1, n)], 1) if n > 1 else np.zeros((0, 2), dtype=np.int64)
    w = _weights(rng, len(eid))
    truth = np.zeros(n, dtype=np.int64)
    un = integer_terms(rng, n, K, truth)
    return finish(Case("tiny-n%d-K%d" % (n, K), n, K, beta, eid, w, un, (np.arange(n) + 1) % K), icm_before_components=False)


_general_cache = {}


def general_cases():
    """name -> Case.  K over {2, 3, 4, 6, 7, 64}: the row loads of the table and chain kernels take 2, 1, 4, 2, 1, 4 floats;
    no n is a multiple of 64."""
    if not _general_cache:
        cases = [knn_case(31, 3001, 4, 3, 1.0), knn_case(32, 2999, 8, 6, 0.5), knn_case(33, 1003, 4, 64, 2.0),
                 sparse_case(34, 5000, 4, 1.0), hub_case(35, 301, 7, 2.0), hub_case(47, 301, 64, 0.5),
                 deg4_case(37, 1003, 2, 2.0), path_case(38, 3, 1.0), tiny_case(1, 2, 1.0), tiny_case(2, 3, 0.5),
                 tiny_case(3, 2, 2.0)]
        for c in cases:
            assert c.n % 64 != 0 and c.n <= 5000
            _general_cache[c.name] = c
    return _general_cache


# ------------------------------------------------------------------------------------------------ incomplete grids
GRID_SHAPES = [(14, 19, False, 3), (33, 70, False, 4), (40, 40, True, 5)]             # H, W, diagonal, K
# removal -> (declared num_neighbor, what goes); an edge's direction is (rows down, columns right) from its smaller end
REMOVALS = ("rand5", "rand15", "rand40", "no-up-right", "no-vertical", "four-on-file", "horizontal-anti", "nn4-rand20")


def stencil_edges(H, W, diagonal, num_neighbor):
    """the complete stencil -> (eid[E,2], direction[E,2] = (di, dj) of the larger end seen from the smaller)"""
    n = H * (H + 1) // 2 if diagonal else H * W
    eid = np.int64(R.grid_edges(np.ones((n, 1)), H, W, diagonal, num_neighbor)[:, :2])
    ii, jj = M.grid_coords(H, W, diagonal)
    d = np.stack([ii[eid[:, 1]] - ii[eid[:, 0]], jj[eid[:, 1]] - jj[eid[:, 0]]], 1)
    return n, eid, d


def grid_case(H, W, diagonal, K, removal, seed, beta):
    declared = 4 if removal.startswith("nn4") else 8
    rng = np.random.default_rng(seed)
    n, eid, d = stencil_edges(H, W, diagonal, declared)
    expected = len(eid)
    horizontal, vertical = (d[:, 0] == 0), (d[:, 0] == 1) & (d[:, 1] == 0)
    anti = (d[:, 0] == 1) & (d[:, 1] == -1)                 # the up-right edge (v, v - W + 1) of its lower end
    if removal.startswith("rand") or removal == "nn4-rand20":
        frac = int(removal.split("rand")[1]) / 100.0
        keep = rng.random(expected) >= frac
        keep[(eid[:, 0] == 0)] = True                        # node 0 keeps its edges: infer_grid reads the geometry off them
    elif removal == "no-up-right":
        keep = ~anti
    elif removal == "no-vertical":
        keep = ~vertical
    elif removal == "four-on-file":
        keep = horizontal | vertical
    else:
        assert removal == "horizontal-anti"
        keep = horizontal | anti
    eid = eid[keep]
    assert len(eid) < expected                               # set_grid will see present < expected: an incomplete grid
    w = _weights(rng, len(eid))
    img = synth.label_image(rng, H, W, K, mean_run=6)
    ii, jj = M.grid_coords(H, W, diagonal)
    truth = img[ii, jj].astype(np.int64)
    region = (ii // 5) * ((W + 4) // 5) + jj // 5
    un = integer_terms(rng, n, K, truth)
    init = blobby_start(rng, K, region, truth, noise=0.25)
    name = "%dx%d%s-%s" % (H, W, "d" if diagonal else "", removal)
    c = finish(Case(name, n, K, beta, eid, w, un, init, grid=(H, W, diagonal, declared)))
    c.expected_edges = expected
    return c


_grid_cache = {}
# seeds of the small cases with few edges gone, chosen so that they discriminate (tests/test_graph_moves_cpu.py asserts it of
# every case): few seeds leave a component there that hangs together by a skipped edge alone
GRID_SEEDS = {(14, "rand5"): 116, (14, "rand15"): 114, (40, "rand5"): 102}


def grid_cases():
    """name -> Case: every shape with every removal (seeds and betas dealt over them)"""
    if not _grid_cache:
        q = 0
        for H, W, diagonal, K in GRID_SHAPES:
            for removal in REMOVALS:
                c = grid_case(H, W, diagonal, K, removal, GRID_SEEDS.get((H, removal), 50 + q), BETAS[(q + q // 8) % 3])
                _grid_cache[c.name] = c
                q += 1
    return _grid_cache


def general_names():
    return ["knn-k4-n3001-K3", "knn-k8-n2999-K6", "knn-k4-n1003-K64", "sparse-n5000-K4", "hub-n301-K7", "hub-n301-K64",
            "deg4-n1003-K2", "path-n2500-K3", "tiny-n1-K2", "tiny-n2-K3", "tiny-n3-K2"]


def grid_names():
    return ["%dx%d%s-%s" % (H, W, "d" if diagonal else "", r) for H, W, diagonal, _ in GRID_SHAPES for r in REMOVALS]


# ------------------------------------------------------------------------------------------------ what the cases discriminate
def components(n, a, b):
    """connected components of the edges (a[i], b[i]) -> canonical ids (smallest node of each component)"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    A = sp.coo_matrix((np.ones(len(a)), (a, b)), shape=(n, n))
    _, comp = connected_components(A, directed=False)
    root = np.full(comp.max() + 1, n, dtype=np.int64)
    np.minimum.at(root, comp, np.arange(n))
    return root[comp]


def true_components(case, labels):
    a, b = case.eid[:, 0], case.eid[:, 1]
    same = labels[a] == labels[b]
    return components(case.n, a[same], b[same])


def shortcut_components(case, labels, rule):
    """The components a complete-stencil argument would give on this edge list.  A node is "linked left" when i - 1 is on its
    row and carries its label; every other node unions with all its smaller equal-label neighbours.
      rule "largest": a linked-left node unions with i - 1 and with its LARGEST remaining smaller neighbour only (the
                      shortcut as the union kernel's comment states it: up-right in an 8-neighbourhood, up in a 4-);
      rule "stencil8": the 8-neighbour refinement of that comment -- a linked-left cell "always has its up-left and up cells
                      above it; a third one is the up-right cell", and it acts only where an upper run STARTS there: with
                      fewer than three smaller neighbours besides i - 1, or when the one before the largest carries the
                      label, it unions with i - 1 alone."""
    g = case.g
    ua, ub = [], []
    for i in range(case.n):
        row = g.col[g.row_ptr[i]:g.row_ptr[i + 1]]
        small = row[row < i]
        linked = len(small) and small[-1] == i - 1 and labels[i - 1] == labels[i]
        if linked:
            ua.append(i)
            ub.append(i - 1)
            above = small[:-1]
            take = above[-1:]
            if rule == "stencil8" and (len(above) < 3 or labels[above[-2]] == labels[i]):
                take = above[:0]
        else:
            take = small
        for c in take:
            if labels[c] == labels[i]:
                ua.append(i)
                ub.append(int(c))
    return components(case.n, np.asarray(ua, dtype=np.int64), np.asarray(ub, dtype=np.int64))


# ------------------------------------------------------------------------------------------------ path families
def launch_violations(g, segments, min_len=2, max_len=63):
    """What makes the segments of ONE launch of the chain kernel unsafe -> list of findings (empty: safe).  The exact 1-D move
    holds every node outside a segment fixed and knows of no edge inside it but the links between consecutive nodes, and the
    segments of a launch move at the same time: so every segment must be an INDUCED path of min_len .. max_len nodes, no
    node may occur twice and no edge may join two segments."""
    bad = []
    owner = -np.ones(g.n, dtype=np.int64)
    pos = -np.ones(g.n, dtype=np.int64)
    for s, seg in enumerate(segments):
        seg = np.asarray(seg, dtype=np.int64)
        if not min_len <= len(seg) <= max_len:
            bad.append(("length", s, len(seg)))
        if seg.min() < 0 or seg.max() >= g.n:
            bad.append(("node out of range", s))
            continue
        if (owner[seg] >= 0).any() or len(np.unique(seg)) != len(seg):
            bad.append(("node twice", s))
        owner[seg] = s
        pos[seg] = np.arange(len(seg))
    so, do = owner[g.src], owner[g.col]
    inside = (so >= 0) & (so == do)
    gap = np.abs(pos[g.src] - pos[g.col])
    if (inside & (gap != 1)).any():
        bad.append(("edge between nodes of a segment that are not consecutive", int(so[inside & (gap != 1)][0])))
    if ((so >= 0) & (do >= 0) & (so != do)).any():
        bad.append(("edge between two segments", int(so[(so >= 0) & (do >= 0) & (so != do)][0])))
    keys = set((g.src * g.n + g.col).tolist())
    for s, seg in enumerate(segments):
        seg = np.asarray(seg, dtype=np.int64)
        if any(int(a) * g.n + int(b) not in keys for a, b in zip(seg[:-1], seg[1:])):
            bad.append(("consecutive nodes not adjacent", s))
    return bad


def greedy_induced_paths(g, rng, max_len=63):
    """One colour of induced, mutually non-adjacent paths of a graph (the rule the library's path families follow: a path
    grows at either end by a node that has exactly ONE neighbour among the nodes taken so far) -> list of node arrays of
    2 .. max_len nodes.  A CPU stand-in for the library's tables, for the tests of the model and of launch_violations."""
    taken = np.zeros(g.n, dtype=bool)
    cnt = np.zeros(g.n, dtype=np.int64)
    out = []

    def take(v):
        taken[v] = True
        cnt[g.col[g.row_ptr[v]:g.row_ptr[v + 1]]] += 1

    for s0 in rng.permutation(g.n):
        if taken[s0] or cnt[s0]:
            continue
        path = [int(s0)]
        take(s0)
        for side in (0, 1):
            while len(path) < max_len:
                e = path[-1] if side == 0 else path[0]
                cand = [int(u) for u in g.col[g.row_ptr[e]:g.row_ptr[e + 1]] if not taken[u] and cnt[u] == 1]
                if not cand:
                    break
                v = cand[int(rng.integers(0, len(cand)))]
                take(v)
                path = path + [v] if side == 0 else [v] + path
        if len(path) >= 2:
            out.append(np.asarray(path, dtype=np.int64))
    return out


def chain_move_on_segments(case, labels, segments):
    """the model's exact chain move on the segments of one launch, in place -> labels changed"""
    if not len(segments):
        return 0
    nodes, lens, _, _ = M.pack_family((list(segments), np.zeros(len(segments), dtype=np.int64), 1))
    return M.chain_move(case.g, case.un, labels, case.beta, nodes, lens, np.ones(len(segments), dtype=bool))


def grid_segments(case, family, phase, colour):
    """the segments of one launch of the chain kernel on a grid block, by the model's families: chains of the colour cut at
    the separators 63, 127, ... (phase 0) or 31, 95, ... (phase 1) of the chain"""
    H, W, diagonal, nn = case.grid
    chains, colours, _ = M.chain_families(H, W, diagonal, nn)[family]
    segs = []
    for ch, cc in zip(chains, colours):
        if cc != colour:
            continue
        start, sep = 0, (31 if phase else 63)
        while start < len(ch):
            end = min(sep, len(ch))
            if end > start:
                segs.append(np.asarray(ch[start:end], dtype=np.int64))
            start = sep + 1
            sep += 64
    return segs
