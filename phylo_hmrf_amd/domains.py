"""The domains of ONE state map: where the blocks of each state lie, and which states border which.

`state_domains(state_vec, len_vec, conf=None, min_area=None)` lists, region by region, the DOMAINS of the map -- the
8-connected components of equal state on a region's full matrix, with the smoothing's area and mirror-twin conventions --
with their bounding box, area, boundary and distance range (phmrf_state_domains, csrc/domains.hip), and counts the edges of
the regions' 8-neighbour grid graphs per pair of states (phmrf_state_adjacency): the length of the interface between two
states, which is what the Potts term of the model pays for.  `domain_lines(...)` writes the table in genome coordinates,
`domains_files(...)` is the command line's --domains FILE.mat.

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os

import numpy as np

from .compare import count_pairs
from .maps import (CONF_ONE, FIRST_CAPACITY, check_len_vec, check_state_vec, conf_array, default_max_area, device, list_rows,
                   load_map, regions, stem)

STATE_DOMAIN_COLS = 16           # include/phmrf.h PHMRF_STATE_DOMAIN_COLS
GRID_CAP = 1024                  # csrc/domains.hip DOM_GRID_CAP: workgroups (of 256 lanes) of its kernels
SUMMARY_COLS = ("nodes", "components", "domains", "domain_nodes", "largest_area", "boundary_edges")
HEADER = ("#chrom1\tstart1\tstop1\tchrom2\tstart2\tstop2\tstate\tarea\tnodes\tconf\tboundary\tneighbour\tneighbour_edges"
          "\tdist_min\tdist_max\n")


def state_domains(state_vec, len_vec, conf=None, min_area=None):
    """Region by region -> dict:
      domains int64 [D, 17]              the region's row in len_vec, then the 16 columns of phmrf_state_domains
      domain_conf float64 [D]            the domains' mean confidence (NaN without conf)
      domain_vec int32 [n]               the row of `domains` a node belongs to, -1 for a node of no listed domain
      adjacency int64 [K, K], adjacency_region [R, K, K]   stored edges per pair of states (symmetric; the diagonal: inside)
      components int64 [R, K]            all components per state, whatever their area
      state_summary int64 [K, 6]         SUMMARY_COLS: nodes, components, listed domains, nodes in listed domains, the largest
                                         listed area, boundary edges (the adjacency row without its diagonal)
    min_area=None lists the domains the small-region smoothing would not call small: area >= default_max_area(H) + 1."""
    import torch
    from . import _lib
    s = check_state_vec(state_vec)
    L = check_len_vec(len_vec, s.shape[0])
    if min_area is not None and int(min_area) < 1:
        raise ValueError("min_area must be >= 1 (None: the smoothing's area rule + 1)")
    n, R = s.shape[0], L.shape[0]
    conf = None if conf is None else conf_array(conf, n, "conf")
    K = int(s.max()) + 1 if n else 1
    lib, dev, stream = device()
    s_t = torch.from_numpy(s.astype(np.uint8)).to(dev)
    c_t = None if conf is None else torch.from_numpy(conf).to(dev)
    out_t = torch.full((n,), -1, dtype=torch.int32, device=dev)
    adjacency = np.zeros((R, K, K), dtype=np.int64)
    components = np.zeros((R, K), dtype=np.int64)
    nodes = np.zeros(K, dtype=np.int64)
    rows, offset = [], 0
    null = ctypes.c_void_p(None)
    for r, lo, hi, H, W, diag, dist0 in regions(L):
        area = default_max_area(H) + 1 if min_area is None else int(min_area)
        labels = ctypes.c_void_p(s_t[lo:hi].data_ptr())
        _lib.check(lib.phmrf_state_adjacency(labels, H, W, diag, K, _lib.ptr_i64(adjacency[r]), stream))
        nodes += np.diagonal(count_pairs(lib, stream, s_t[lo:hi], s_t[lo:hi], K, K))

        def call(capacity, table, found):
            _lib.check(lib.phmrf_state_domains(
                labels, null if c_t is None else ctypes.c_void_p(c_t[lo:hi].data_ptr()), H, W, diag, dist0,
                K, area, ctypes.c_void_p(out_t[lo:hi].data_ptr()), capacity, _lib.ptr_i64(table), ctypes.byref(found),
                _lib.ptr_i64(components[r]), stream))

        table = list_rows(call, STATE_DOMAIN_COLS, FIRST_CAPACITY)
        if offset:
            view = out_t[lo:hi]
            view[view >= 0] += offset
        offset += table.shape[0]
        rows.append(np.concatenate([np.full((table.shape[0], 1), r, dtype=np.int64), table], axis=1))
    domains = np.concatenate(rows) if rows else np.zeros((0, STATE_DOMAIN_COLS + 1), dtype=np.int64)
    if conf is None:
        domain_conf = np.full(domains.shape[0], np.nan)
    else:
        domain_conf = domains[:, 14].astype(np.float64) / (domains[:, 6].astype(np.float64) * CONF_ONE)
    total = adjacency.sum(axis=0)
    return dict(domains=domains, domain_conf=domain_conf, domain_vec=out_t.cpu().numpy(), adjacency=total,
                adjacency_region=adjacency, components=components,
                state_summary=state_summary(domains, total, components, nodes))


def state_summary(domains, adjacency, components, nodes):
    """-> int64 [K, 6] (SUMMARY_COLS) from the results of the regions.  Host only."""
    K = adjacency.shape[0]
    out = np.zeros((K, len(SUMMARY_COLS)), dtype=np.int64)
    state = domains[:, 8]
    out[:, 0] = nodes
    out[:, 1] = np.asarray(components).reshape(-1, K).sum(axis=0)
    out[:, 2] = np.bincount(state, minlength=K)
    np.add.at(out[:, 3], state, domains[:, 6])
    np.maximum.at(out[:, 4], state, domains[:, 7])
    out[:, 5] = adjacency.sum(axis=1) - np.diagonal(adjacency)
    return out


def domain_lines(domains, domain_conf, len_vec, resolution):
    """-> the lines of domains_*.txt, header first: the bounding boxes in genome coordinates (compare_domains_*.txt's), the
    states 1-based (neighbour 0: the domain borders no other state), the distance range in bp"""
    res = int(resolution)
    lines = [HEADER]
    for d, c in zip(np.asarray(domains), np.asarray(domain_conf).reshape(-1)):
        row = len_vec[int(d[0])]
        s1, s2 = int(row[5]), int(row[6])
        lines.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t%d\t%d\t%d\t%d\t%d\n"
                     % (row[9], (s1 + d[2]) * res, (s1 + d[3] + 1) * res, row[9], (s2 + d[4]) * res, (s2 + d[5] + 1) * res,
                        d[8] + 1, d[7], d[6], c, d[9], d[10] + 1, d[11], d[12] * res, d[13] * res))
    return lines


def domains_files(path, output_path, resolution, field="state_vec", min_area=None):
    """The command line's --domains: list the domains of the `field` of one .mat, write domains_<stem>.mat and
    domains_<stem>.txt under output_path.  -> the .mat"""
    import scipy.io
    if int(resolution) < 1:
        raise ValueError("resolution must be >= 1")
    s, L, conf = load_map(path, field)
    res = state_domains(s, L, conf, min_area=min_area)
    os.makedirs(output_path, exist_ok=True)
    areas = np.array([default_max_area(r[3]) + 1 if min_area is None else int(min_area) for r in L], dtype=np.int64)
    out = os.path.join(output_path, "domains_%s.mat" % stem(path))
    scipy.io.savemat(out, dict(res, len_vec=L, domains_field=field, domains_area=areas, resolution=int(resolution)))
    with open(os.path.join(output_path, "domains_%s.txt" % stem(path)), "wb") as fh:
        fh.write("".join(domain_lines(res["domains"], res["domain_conf"], L, resolution)).encode())
    return out
