"""Plain NumPy / SciPy restatement of the comparison of two state maps (phylo_hmrf_amd.compare, csrc/compare.hip), on the
FULL matrix of a region -- the yardstick of the GPU calls, which work on the stored nodes alone.

  - contingency: stored nodes per (state in A, state in B);
  - diff codes: 0 where a == map_b[b], else 2 where both float32 confidences are >= float32(min_conf) (always, with no
    confidences or min_conf <= 0), else 1;
  - domains: scipy.ndimage.label with the 3 x 3 structure on the full matrix of diff == 2.  A component's area is its pixel
    count on the full matrix.  A diagonal block's component that lies wholly below the diagonal is the twin of one above it
    and is dropped; every other component is described by its STORED nodes (upper triangle): root = the smallest node id,
    bounding box, node count, the most frequent states (np.argmax of the histogram: the lowest on ties) and the sums of
    floor(float64(float32(conf)) * 2^24);
  - bands: per band of d = |dist0 + j - i| (0: d == 0; t >= 1: 2^(t-1) <= d < 2^t) the nodes, those with diff >= 1 and
    those with diff == 2.
"""
import numpy as np
from scipy import ndimage

from tests.smooth_reference import default_max_area, full_matrix

BANDS = 32
COLS = 12


def contingency(a, b, KA, KB):
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    assert a.size == 0 or (a.max() < KA and b.max() < KB)
    return np.bincount(a * KB + b, minlength=KA * KB).reshape(KA, KB)


def mapped(b, map_b):
    b = np.asarray(b, dtype=np.int64).reshape(-1)
    return b if map_b is None else np.asarray(map_b, dtype=np.int64)[b]


def diff_codes(a, b, map_b=None, conf_a=None, conf_b=None, min_conf=0.0):
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    differ = a != mapped(b, map_b)
    counts = np.ones(a.shape, dtype=bool)
    if conf_a is not None and min_conf > 0:
        m = np.float32(min_conf)
        counts = (np.asarray(conf_a, dtype=np.float32) >= m) & (np.asarray(conf_b, dtype=np.float32) >= m)
    return np.where(differ, np.where(counts, 2, 1), 0).astype(np.uint8)


def node_coords(H, W, diagonal):
    if diagonal:
        return np.triu_indices(H)
    i, j = np.divmod(np.arange(H * W), W)
    return i, j


def fixed(conf):
    return np.floor(np.asarray(conf, dtype=np.float32).astype(np.float64) * float(1 << 24)).astype(np.int64)


def domains(a, b, diff, H, W, diagonal, min_area, map_b=None, conf_a=None, conf_b=None):
    """-> int64 [D, 12], the listed domains in ascending order of their roots"""
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    bm = mapped(b, map_b)
    lab, nc = ndimage.label(full_matrix(np.asarray(diff) == 2, H, W, diagonal), structure=np.ones((3, 3), dtype=bool))
    area = np.bincount(lab.reshape(-1), minlength=nc + 1)
    ii, jj = node_coords(H, W, diagonal)
    of_node = lab[ii, jj]                                   # the component of every stored node
    fa = fixed(conf_a) if conf_a is not None else np.zeros(a.shape, dtype=np.int64)
    fb = fixed(conf_b) if conf_b is not None else np.zeros(a.shape, dtype=np.int64)
    KA, KM = int(a.max()) + 1, int(bm.max()) + 1
    order = np.argsort(of_node, kind="stable")              # the stored nodes component by component, ascending ids within
    order = order[of_node[order] > 0]
    first = np.nonzero(np.diff(of_node[order], prepend=0))[0]
    rows = []
    for lo, hi in zip(first, np.append(first[1:], order.size)):      # (a component wholly below the diagonal, the twin of a
        v = order[lo:hi]                                             #  listed one, has no stored node and does not occur)
        c = of_node[v[0]]
        if area[c] < min_area:
            continue
        rows.append([v.min(), ii[v].min(), ii[v].max(), jj[v].min(), jj[v].max(), v.size, area[c],
                     int(np.argmax(np.bincount(a[v], minlength=KA))), int(np.argmax(np.bincount(bm[v], minlength=KM))),
                     fa[v].sum(), fb[v].sum(), 0])
    rows.sort(key=lambda r: r[0])
    return np.array(rows, dtype=np.int64).reshape(-1, COLS)


def band_of(d):
    return np.searchsorted(2 ** np.arange(BANDS, dtype=np.int64), np.asarray(d, dtype=np.int64), side="right")


def bands(diff, H, W, diagonal, dist0):
    ii, jj = node_coords(H, W, diagonal)
    t = band_of(np.abs(dist0 + jj.astype(np.int64) - ii))
    diff = np.asarray(diff)
    out = np.zeros((BANDS, 3), dtype=np.int64)
    out[:, 0] = np.bincount(t, minlength=BANDS)
    out[:, 1] = np.bincount(t[diff >= 1], minlength=BANDS)
    out[:, 2] = np.bincount(t[diff == 2], minlength=BANDS)
    return out


def compare_region(a, b, H, W, diagonal, dist0=0, min_area=1, map_b=None, conf_a=None, conf_b=None, min_conf=0.0):
    """-> (diff uint8 [n], domains int64 [D, 12], bands int64 [32, 3])"""
    diff = diff_codes(a, b, map_b, conf_a, conf_b, min_conf)
    return diff, domains(a, b, diff, H, W, diagonal, min_area, map_b, conf_a, conf_b), bands(diff, H, W, diagonal, dist0)


def compare_state_vec(a, b, len_vec, map_b=None, conf_a=None, conf_b=None, min_conf=0.0, min_area=None):
    """-> (diff_vec, domains int64 [D, 13] with the region's row number first, bands [R, 32, 3])"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    diff_vec = np.zeros(a.shape, dtype=np.uint8)
    tables, all_bands = [], []
    for r, row in enumerate(np.atleast_2d(np.asarray(len_vec))):
        lo, hi, H, W, diag = int(row[1]), int(row[2]), int(row[3]), int(row[4]), int(row[8]) == 1
        area = default_max_area(H) + 1 if min_area is None else min_area
        ca = None if conf_a is None else np.asarray(conf_a).reshape(-1)[lo:hi]
        cb = None if conf_b is None else np.asarray(conf_b).reshape(-1)[lo:hi]
        d, t, bd = compare_region(a[lo:hi], b[lo:hi], H, W, diag, int(row[6]) - int(row[5]), area, map_b, ca, cb, min_conf)
        diff_vec[lo:hi] = d
        tables.append(np.concatenate([np.full((t.shape[0], 1), r, dtype=np.int64), t], axis=1))
        all_bands.append(bd)
    return diff_vec, np.concatenate(tables), np.stack(all_bands)
