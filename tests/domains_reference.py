"""Plain NumPy / SciPy restatement of the domains of one state map (phylo_hmrf_amd.domains, csrc/domains.hip), on the FULL
matrix of a region -- the yardstick of the GPU calls, which work on the stored nodes alone.

  - adjacency: np.bincount over the edge list of graph_host.grid_edges(..., num_neighbor=8) -- the definition is the graph's
    own --, folded into the symmetric table (the diagonal: the edges inside one state);
  - domains: scipy.ndimage.label with the 3 x 3 structure on the full matrix, state by state.  A component's area is its
    pixel count on the full matrix.  A diagonal block's component that lies wholly below the diagonal is the twin of one
    above it and does not occur; every other component is described by its STORED nodes (upper triangle): root = the
    smallest node id, bounding box, node count, state, the stored edges that leave it for another state (total, the state
    that holds most of them -- np.argmax: the lowest on ties --, the edges to it), the range of d = |dist0 + j - i| and the
    sum of floor(float64(float32(conf)) * 2^24);
  - listed: area >= min_area, in ascending order of the roots.
"""
import functools

import numpy as np
from scipy import ndimage

from phylo_hmrf_amd import graph_host
from tests.compare_reference import fixed, node_coords
from tests.smooth_reference import default_max_area, full_matrix

COLS = 16


@functools.lru_cache(maxsize=4)
def edges(H, W, diagonal):
    """-> (u, v) int64: the stored edges of the region's 8-neighbour grid graph, each once (shared: not to be written to)"""
    n = H * (H + 1) // 2 if diagonal else H * W
    e = graph_host.grid_edges(np.zeros((n, 1)), H, W, bool(diagonal), num_neighbor=8)
    return e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)


def adjacency(states, H, W, diagonal, K):
    s = np.asarray(states, dtype=np.int64).reshape(-1)
    u, v = edges(H, W, diagonal)
    raw = np.bincount(s[u] * K + s[v], minlength=K * K).reshape(K, K)
    return raw + raw.T - np.diag(np.diagonal(raw))


def region(states, H, W, diagonal, K, dist0=0, min_area=1, conf=None):
    """-> dict(table int64 [D, 16], n_components int64 [K], domain_out int32 [n], all_boundary: the boundary edges of ALL
    components summed)"""
    s = np.asarray(states, dtype=np.int64).reshape(-1)
    n = s.size
    M = full_matrix(s, H, W, diagonal)
    lab = np.zeros(M.shape, dtype=np.int64)
    total = 0
    for k in np.unique(M):
        one, nc = ndimage.label(M == k, structure=np.ones((3, 3), dtype=bool))
        lab[one > 0] = one[one > 0] + total
        total += nc
    area_full = np.bincount(lab.reshape(-1), minlength=total + 1)
    ii, jj = node_coords(H, W, diagonal)
    ii, jj = np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64)
    uniq, inv = np.unique(lab[ii, jj], return_inverse=True)      # the components with a stored node
    inv = inv.reshape(-1)
    C = uniq.size
    v = np.arange(n, dtype=np.int64)
    big = np.iinfo(np.int64).max

    def lowest(x):
        out = np.full(C, big, dtype=np.int64)
        np.minimum.at(out, inv, x)
        return out

    def highest(x):
        out = np.full(C, -1, dtype=np.int64)
        np.maximum.at(out, inv, x)
        return out

    root = lowest(v)
    d = np.abs(dist0 + jj - ii)
    eu, ev = edges(H, W, diagonal)
    leave = s[eu] != s[ev]
    frm, to = np.concatenate([eu[leave], ev[leave]]), np.concatenate([ev[leave], eu[leave]])
    hist = np.bincount(inv[frm] * K + s[to], minlength=C * K).reshape(C, K)
    boundary = hist.sum(axis=1)
    towards = np.where(boundary > 0, np.argmax(hist, axis=1), -1)
    csum = np.zeros(C, dtype=np.int64)
    if conf is not None:
        np.add.at(csum, inv, fixed(conf))
    table = np.stack([root, lowest(ii), highest(ii), lowest(jj), highest(jj), np.bincount(inv, minlength=C), area_full[uniq],
                      s[root], boundary, towards, hist.max(axis=1), lowest(d), highest(d), csum, np.zeros(C, dtype=np.int64),
                      np.zeros(C, dtype=np.int64)], axis=1).astype(np.int64)
    keep = np.flatnonzero(table[:, 6] >= min_area)
    keep = keep[np.argsort(root[keep], kind="stable")]
    ident = np.full(C, -1, dtype=np.int64)
    ident[keep] = np.arange(keep.size)
    return dict(table=table[keep].reshape(-1, COLS), n_components=np.bincount(s[root], minlength=K),
                domain_out=ident[inv].astype(np.int32), all_boundary=int(boundary.sum()))


def state_vec_domains(state_vec, len_vec, conf=None, min_area=None):
    """-> the dict of phylo_hmrf_amd.domains.state_domains"""
    s = np.asarray(state_vec, dtype=np.int64).reshape(-1)
    L = np.atleast_2d(np.asarray(len_vec)).astype(np.int64)
    K = int(s.max()) + 1
    tables, adj, comps = [], [], []
    domain_vec = np.full(s.size, -1, dtype=np.int32)
    offset = 0
    for r, row in enumerate(L):
        lo, hi, H, W, diag = int(row[1]), int(row[2]), int(row[3]), int(row[4]), int(row[8]) == 1
        area = default_max_area(H) + 1 if min_area is None else min_area
        c = None if conf is None else np.asarray(conf).reshape(-1)[lo:hi]
        got = region(s[lo:hi], H, W, diag, K, int(row[6]) - int(row[5]), area, c)
        t = got["table"]
        domain_vec[lo:hi] = np.where(got["domain_out"] >= 0, got["domain_out"] + offset, -1)
        offset += t.shape[0]
        tables.append(np.concatenate([np.full((t.shape[0], 1), r, dtype=np.int64), t], axis=1))
        adj.append(adjacency(s[lo:hi], H, W, diag, K))
        comps.append(got["n_components"])
    domains = np.concatenate(tables)
    adj, comps = np.stack(adj), np.stack(comps)
    total = adj.sum(axis=0)
    if conf is None:
        domain_conf = np.full(domains.shape[0], np.nan)
    else:
        domain_conf = domains[:, 14] / (domains[:, 6] * float(1 << 24))
    summary = np.zeros((K, 6), dtype=np.int64)
    for k in range(K):
        mine = domains[domains[:, 8] == k]
        summary[k] = [(s == k).sum(), comps[:, k].sum(), mine.shape[0], mine[:, 6].sum(), mine[:, 7].max() if mine.size else 0,
                      total[k].sum() - total[k, k]]
    return dict(domains=domains, domain_conf=domain_conf, domain_vec=domain_vec, adjacency=total, adjacency_region=adj,
                components=comps, state_summary=summary)


def lines(domains, domain_conf, len_vec, resolution):
    """-> the text of domains_*.txt"""
    out = ["#chrom1\tstart1\tstop1\tchrom2\tstart2\tstop2\tstate\tarea\tnodes\tconf\tboundary\tneighbour\tneighbour_edges"
           "\tdist_min\tdist_max\n"]
    for d, c in zip(domains, domain_conf):
        row = np.atleast_2d(len_vec)[int(d[0])]
        chrom, b1, b2 = int(row[9]), int(row[5]), int(row[6])
        cells = [chrom, (b1 + d[2]) * resolution, (b1 + d[3] + 1) * resolution, chrom, (b2 + d[4]) * resolution,
                 (b2 + d[5] + 1) * resolution, d[8] + 1, d[7], d[6], "%.6f" % c, d[9], d[10] + 1, d[11], d[12] * resolution,
                 d[13] * resolution]
        out.append("\t".join(str(int(x)) if not isinstance(x, str) else x for x in cells) + "\n")
    return "".join(out)
