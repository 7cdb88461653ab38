"""CPU: tests/energy_reference.py -- the float64 reference the GPU energy tests (tests/test_gpu_energy.py) assert equality
with -- against the oracle's energy functions, and its own three forms against each other.  Lattice inputs (halves, eighths,
beta in BETAS): every comparison here is exact."""
import numpy as np
import pytest

from oracle import mrf_moves as M
from oracle import ref_numpy as R
from tests import energy_reference as E

# H, W, diagonal, num_neighbor, K, edges removed
GRIDS = [(7, 11, False, 8, 5, 0), (7, 11, False, 4, 3, 0), (12, 12, True, 8, 4, 0), (12, 12, True, 4, 2, 0),
         (1, 9, False, 8, 2, 0), (9, 1, False, 8, 3, 0), (2, 2, True, 8, 2, 0), (10, 13, False, 8, 6, 1), (14, 14, True, 8, 3, 1),
         (16, 9, False, 8, 64, 5)]


def _problem(case, seed=0):
    H, W, diagonal, nn, K, removed = case
    n, eid, w, un = E.lattice_problem(seed + H * 100 + W, H, W, K, diagonal, nn)
    rng = np.random.default_rng(seed + 7)
    if removed:                                        # a grid with missing edges: the reference takes any edge list
        keep = np.ones(len(eid), dtype=bool)
        keep[rng.choice(len(eid), removed, replace=False)] = False
        eid, w = eid[keep], w[keep]
    ii, _ = E.grid_rows_cols(H, W, diagonal)
    return n, eid, w, un, ii, rng


@pytest.mark.parametrize("case", GRIDS)
@pytest.mark.parametrize("beta", E.BETAS)
def test_energy_equals_the_oracles(case, beta):
    H, W, diagonal, nn, K, _ = case
    n, eid, w, un, ii, rng = _problem(case)
    assert E.is_lattice(w, un, beta)
    g = M.Graph(n, eid, w)
    for kind in ("constant", "random", "checkerboard", "absent"):
        lab = E.labelling(kind, rng, H, W, diagonal, K)
        eu, ep = E.energy(eid, w, un, lab)
        assert (eu + beta * ep, eu, beta * ep) == M.energy(g, un, lab, beta)
        assert (eu + beta * ep, eu, beta * ep) == R.mrf_energy(lab, -un, eid, w, beta)
        assert (eu, ep) == E.adjacency_energy(eid, w, un, lab)
        if kind == "constant":
            assert ep == 0.0
        if kind == "checkerboard" and (K >= 4 or nn == 4) and K > 1:
            assert ep == float(np.sum(w))               # every edge is cut


@pytest.mark.parametrize("case", GRIDS)
def test_the_two_forms_of_the_difference_agree_exactly(case):
    H, W, diagonal, nn, K, _ = case
    n, eid, w, un, ii, rng = _problem(case, seed=1)
    a = E.labelling("random", rng, H, W, diagonal, K)
    one = a.copy()
    one[n // 2] = (one[n // 2] + 1) % K
    some = a.copy()
    idx = rng.choice(n, max(1, n // 40), replace=False)
    some[idx] = rng.integers(0, K, idx.size)
    for b in (a, one, some, (a + 1) % K):
        for rows in (None, (0, H), (H // 3, H - H // 3)):
            direct, local = E.energy_difference(eid, w, un, a, b, ii, rows)
            assert direct == local, (rows, direct, local)
            back, _ = E.energy_difference(eid, w, un, b, a, ii, rows)
            assert back == (-direct[0], -direct[1])
        if b is a:
            assert direct == (0.0, 0.0)


@pytest.mark.parametrize("case", [c for c in GRIDS if c[0] >= 7])
@pytest.mark.parametrize("parts", [2, 3])
def test_owned_row_sums_of_the_tiles_add_up_to_the_block(case, parts):
    H, W, diagonal, nn, K, _ = case
    n, eid, w, un, ii, rng = _problem(case, seed=2)
    lab = E.labelling("random", rng, H, W, diagonal, K)
    cuts = [0] + [H * p // parts for p in range(1, parts)] + [H]
    ranges = list(zip(cuts, cuts[1:]))
    sums = E.tile_sums(eid, w, un, lab, ii, ranges)
    whole = E.energy(eid, w, un, lab)
    assert (sum(s[0] for s in sums), sum(s[1] for s in sums)) == whole
    # an edge belongs to its upper / left end: the cut edges are the UPPER tile's, so a tile's own stored rows -- its owned rows
    # and one halo row on either side -- hold everything its sums need, and its lower halo's labels enter them
    for t, (r0, r1) in enumerate(ranges):
        s0, s1 = r0 - (t > 0), r1 + (t < parts - 1)
        node0, e_loc, w_loc, un_loc, row_loc = E.tile_local(eid, w, un, H, W, diagonal, s0, s1)
        stored = lab[node0:node0 + len(row_loc)]
        assert E.energy(e_loc, w_loc, un_loc, stored, row_loc, (r0 - s0, r1 - s0)) == sums[t]
        if t < parts - 1 and W > 1:
            other = stored.copy()
            halo = np.flatnonzero(row_loc == s1 - 1 - s0)
            other[halo] = (other[halo] + 1) % K
            d, loc = E.energy_difference(e_loc, w_loc, un_loc, other, stored, row_loc, (r0 - s0, r1 - s0))
            assert d == loc and d[0] == 0.0                      # no owned unary term moves with the halo's labels
        if t > 0:
            other = stored.copy()
            halo = np.flatnonzero(row_loc == 0)
            other[halo] = (other[halo] + 1) % K
            assert E.energy(e_loc, w_loc, un_loc, other, row_loc, (r0 - s0, r1 - s0)) == sums[t]   # the upper halo: nothing of it
