"""GPU: the pile-up of one state map around centres (phmrf_state_pileup, phylo_hmrf_amd.pileup) against the restatement of
tests/pileup_reference.py, which loops over centres and pile cells as the definition reads.  Everything is integer arithmetic:
every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

from phylo_hmrf_amd import pileup
from tests import pileup_reference as R

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4
FILL = 0xA5
DIAGONAL = (1, 2, 7, 65, 130)
OFF_DIAGONAL = ((1, 1), (1, 9), (7, 13), (70, 33))
FLANKS = (0, 1, 3, 8)                                         # 8: 289 pile cells, a second tile of 256


@pytest.fixture(scope="module")
def gpu():
    import torch
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    return L, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _call(gpu, labels, H, W, diag, K, w, G, offsets, ci, cj, orient=None, offset=0, null=(), small=False):
    """-> (status, obs): obs int64 [G, 2w + 1, 2w + 1, K] after a call that succeeded, else the flat buffer, which is filled
    with FILL before the call.  The labels start `offset` bytes into their device buffer.  null: names of pointers passed as
    NULL.  small: a call that must be refused, with a one-word buffer."""
    import torch
    L, dev, st = gpu
    side = 2 * max(w, 0) + 1
    count = 1 if small else max(1, max(G, 1) * side * side * max(K, 1))
    obs = np.full(8 * count, FILL, dtype=np.uint8).view(np.int64)
    a = np.zeros(offset + len(labels), dtype=np.uint8)
    a[offset:] = labels
    held = [torch.from_numpy(a).to(dev)[offset:]]

    def up(name, x, dtype):
        if x is None or name in null:
            return None
        held.append(torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(dev))
        return ctypes.c_void_p(held[-1].data_ptr())

    off = np.ascontiguousarray(offsets, dtype=np.int64)
    status = L.phmrf_state_pileup(None if "labels" in null else ctypes.c_void_p(held[0].data_ptr()), H, W, int(diag), K, w, G,
                                  None if "offsets" in null else off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  up("ci", ci, np.int32), up("cj", cj, np.int32), up("orient", orient, np.uint8),
                                  None if "obs" in null else obs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), st)
    if status == 0 and not small:
        obs = obs[:G * side * side * K].reshape(G, side, side, K)
    return status, obs


def _untouched(obs):
    return bool(np.all(obs.view(np.uint8) == FILL))


def _in_range(H, W, w, G, offsets, ci, cj, orient):
    """-> int64 [G, 2w + 1, 2w + 1]: the centres of group g whose pile cell lies inside the region, from the geometry alone"""
    n = int(offsets[G])
    ci, cj = np.asarray(ci[:n], dtype=np.int64)[:, None, None], np.asarray(cj[:n], dtype=np.int64)[:, None, None]
    o = (np.zeros(n, dtype=np.int64) if orient is None else np.asarray(orient[:n], dtype=np.int64))[:, None, None]
    u, v = np.arange(-w, w + 1)[None, :, None], np.arange(-w, w + 1)[None, None, :]
    p, q = np.where(o & 2, v, u), np.where(o & 2, u, v)
    s = 1 - 2 * (o & 1)
    inside = (ci + s * p >= 0) & (ci + s * p < H) & (cj + s * q >= 0) & (cj + s * q < W)
    out = np.zeros((G, 2 * w + 1, 2 * w + 1), dtype=np.int64)
    for g in range(G):
        out[g] = inside[int(offsets[g]):int(offsets[g + 1])].sum(axis=0)
    return out


def _check(gpu, labels, H, W, diag, K, w, G, offsets, ci, cj, orient=None, offset=0, what="", ref=None):
    status, obs = _call(gpu, labels, H, W, diag, K, w, G, offsets, ci, cj, orient, offset)
    what = (what, H, W, diag, K, w, G, list(offsets), offset)
    assert status == 0, what
    want = R.table(labels, H, W, diag, K, w, G, offsets, np.asarray(ci), np.asarray(cj), orient) if ref is None else ref
    assert obs.shape == want.shape and np.array_equal(obs, want), (what, np.argwhere(obs != want)[:5].tolist())
    assert np.array_equal(obs.sum(axis=-1), _in_range(H, W, w, G, offsets, ci, cj, orient)), what
    return obs


# ---- maps and centres -------------------------------------------------------------------------------------------------------
def _nodes(M, diag):
    M = np.asarray(M)
    return (M[np.triu_indices(M.shape[0])] if diag else M.reshape(-1)).astype(np.uint8)


KINDS = ("random", "blocky", "constant", "rows")


def _map(kind, H, W, diag, K, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        M = rng.integers(0, K, (H, W))
    elif kind == "blocky":                                   # constant tiles of 1 - 9 rows by 1 - 9 columns
        rows = np.repeat(np.arange(H), rng.integers(1, 10, H))[:H]
        cols = np.repeat(np.arange(W), rng.integers(1, 10, W))[:W]
        M = rng.integers(0, K, (H, W))[rows][:, cols]
    elif kind == "constant":
        M = np.full((H, W), K - 1)
    elif kind == "rows":                                     # single-row stripes
        M = np.indices((H, W))[0] % K
    else:
        raise ValueError(kind)
    return _nodes(M, diag)


def _centres(H, W, w, G, seed, empty=()):
    """-> (offsets [G + 1], ci, cj, orient): every corner, centres wholly outside (negative and beyond the region), in the
    lower triangle, a duplicate of each of the first four, and seeded ones around the region; the four orientations mixed
    within every group; the groups in `empty` hold nothing"""
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (-w - 1, 0), (0, -w - 5), (H + w, W - 1), (H - 1, W + w + 3),
             (-1000, -1000), (H - 1, 0), (H // 2, 0)]
    fixed += fixed[:4]
    seeded = np.stack([rng.integers(-w - 1, H + w + 1, 12), rng.integers(-w - 1, W + w + 1, 12)], axis=1)
    c = np.concatenate([np.array(fixed, dtype=np.int64), seeded])
    filled = [g for g in range(G) if g not in empty]
    orient = (np.arange(c.shape[0]) // len(filled)) % 4      # a group's members take 0, 1, 2, 3 in turn
    groups = np.array(filled)[np.arange(c.shape[0]) % len(filled)]                  # dealt round the groups that hold any
    order = np.argsort(groups, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(groups, minlength=G))])
    return offsets, c[order, 0], c[order, 1], orient[order]


# ---- shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", DIAGONAL)
def test_diagonal_regions(gpu, side):
    labels = _map("random", side, side, True, 6, side)
    for w in FLANKS:
        offsets, ci, cj, orient = _centres(side, side, w, 3, side + w, empty=(1,))
        obs = _check(gpu, labels, side, side, True, 6, w, 3, offsets, ci, cj, orient)
        assert obs[0].any() and not obs[1].any() and obs[2].any()


@pytest.mark.parametrize("H,W", OFF_DIAGONAL)
def test_off_diagonal_regions(gpu, H, W):
    labels = _map("random", H, W, False, 6, 100 * H + W)
    for w in FLANKS:
        offsets, ci, cj, orient = _centres(H, W, w, 3, H + W + w, empty=(0,))
        obs = _check(gpu, labels, H, W, False, 6, w, 3, offsets, ci, cj, orient)
        assert not obs[0].any() and obs[1].any() and obs[2].any()


@pytest.mark.parametrize("H,W,diag", [(7, 13, False), (1, 1, False), (2, 2, True), (130, 130, True)])
def test_the_widest_window(gpu, H, W, diag):
    """w = 64: 16,641 pile cells in 66 tiles, the last one partly filled; wider than three of the four regions"""
    labels = _map("blocky", H, W, diag, 6, H)
    ci, cj = np.array([0, H - 1, H // 2, -64, H + 63, H + 64]), np.array([0, 0, W - 1, 3 - 64 if W > 3 else -64, W - 1, 0])
    obs = _check(gpu, labels, H, W, diag, 6, 64, 1, [0, 6], ci, cj, np.array([0, 1, 2, 3, 2, 0]))
    assert obs.shape == (1, 129, 129, 6) and obs.any()


@pytest.mark.parametrize("G", [1, 3, 16])
@pytest.mark.parametrize("K", [1, 6, 64])
def test_state_and_group_counts_with_every_map(gpu, K, G):
    """K = 64: the 32 words of a lane's column all in use; K = 1: a single half-word"""
    empty = {1: (), 3: (0, 2), 16: (0, 5, 6, 15)}[G]
    for H, W, diag in ((65, 65, True), (7, 13, False)):
        offsets, ci, cj, orient = _centres(H, W, 3, G, K + G, empty=empty)
        for m, kind in enumerate(KINDS):
            obs = _check(gpu, _map(kind, H, W, diag, K, K + m), H, W, diag, K, 3, G, offsets, ci, cj, orient, what=kind)
            assert all(not obs[g].any() for g in empty)


def test_no_centres_one_centre_and_no_orient(gpu):
    labels = _map("random", 7, 13, False, 6, 1)
    for null in ((), ("ci", "cj", "orient")):
        status, obs = _call(gpu, labels, 7, 13, False, 6, 2, 3, [0, 0, 0, 0], np.zeros(1), np.zeros(1), np.zeros(1), null=null)
        assert status == 0 and obs.shape == (3, 5, 5, 6) and not obs.any()
    obs = _check(gpu, labels, 7, 13, False, 6, 2, 1, [0, 1], np.array([3]), np.array([4]), np.array([3]))
    assert obs.sum() == 25
    offsets, ci, cj, _ = _centres(7, 13, 2, 2, 5)
    a = _check(gpu, labels, 7, 13, False, 6, 2, 2, offsets, ci, cj, None)
    b = _check(gpu, labels, 7, 13, False, 6, 2, 2, offsets, ci, cj, np.zeros(len(ci), dtype=np.uint8))
    assert np.array_equal(a, b)


@pytest.fixture(scope="module")
def crowd():
    """5,000 seeded centres on a 40 x 40 region: group 0 spans 16 chunks of pileup.CHUNK centres, group 2 four, and every
    workgroup of a group adds into the same cells of the table"""
    rng = np.random.default_rng(40)
    assert 4000 > 15 * pileup.CHUNK and 1000 > 3 * pileup.CHUNK
    ci, cj, orient = rng.integers(-4, 44, 5000), rng.integers(-4, 44, 5000), rng.integers(0, 4, 5000)
    labels = {diag: _map("blocky", 40, 40, diag, 20, 41 + diag) for diag in (False, True)}
    offsets = [0, 4000, 4000, 5000]
    return labels, offsets, ci, cj, orient, {d: R.table(labels[d], 40, 40, d, 20, 3, 3, offsets, ci, cj, orient) for d in labels}


@pytest.mark.parametrize("diag", [False, True])
def test_a_group_of_many_chunks(gpu, crowd, diag):
    labels, offsets, ci, cj, orient, want = crowd
    obs = _check(gpu, labels[diag], 40, 40, diag, 20, 3, 3, offsets, ci, cj, orient, ref=want[diag])
    assert obs[0].sum(axis=-1).max() > pileup.CHUNK and not obs[1].any()


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_label_slices_start_at_any_byte(gpu, offset):
    for H, W, diag in ((65, 65, True), (7, 13, False)):
        offsets, ci, cj, orient = _centres(H, W, 3, 2, offset)
        _check(gpu, _map("random", H, W, diag, 20, offset + H), H, W, diag, 20, 3, 2, offsets, ci, cj, orient, offset=offset)


# ---- identities on the device -----------------------------------------------------------------------------------------------
def test_transpose_and_flip_symmetries(gpu):
    H = 65
    labels = _map("blocky", H, H, True, 6, 8)
    offsets, ci, cj, orient = _centres(H, H, 3, 2, 9)
    a = _check(gpu, labels, H, H, True, 6, 3, 2, offsets, ci, cj, orient)
    b = _check(gpu, labels, H, H, True, 6, 3, 2, offsets, cj, ci, orient ^ 2)       # a diagonal region is its own mirror
    assert np.array_equal(a, b)
    for H, W, diag in ((65, 65, True), (70, 33, False)):
        labels = _map("random", H, W, diag, 6, 10)
        offsets, ci, cj, orient = _centres(H, W, 3, 2, 11)
        a = _check(gpu, labels, H, W, diag, 6, 3, 2, offsets, ci, cj, orient)
        b = _check(gpu, labels, H, W, diag, 6, 3, 2, offsets, ci, cj, orient ^ 1)   # the flip reverses both pile axes
        assert np.array_equal(b, a[:, ::-1, ::-1]) and not np.array_equal(a, b)


def test_two_calls_give_equal_bytes(gpu, crowd):
    labels, offsets, ci, cj, orient, _ = crowd
    a = _call(gpu, labels[True], 40, 40, True, 20, 3, 3, offsets, ci, cj, orient)
    b = _call(gpu, labels[True], 40, 40, True, 20, 3, 3, offsets, ci, cj, orient)
    assert a[0] == 0 and b[0] == 0 and a[1].any() and a[1].tobytes() == b[1].tobytes()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refused_arguments_write_nothing(gpu):
    lab = np.zeros(64, dtype=np.uint8)
    c3 = np.array([1, 2, 3])
    ok = dict(labels=lab, H=4, W=5, diag=False, K=3, w=2, G=2, offsets=[0, 1, 3], ci=c3, cj=c3, orient=np.array([0, 1, 3]))
    status, obs = _call(gpu, **ok)
    assert status == 0 and obs.sum() > 0
    big = 1 << 30
    cases = [
        (dict(null=("labels",)), INVALID), (dict(null=("offsets",)), INVALID), (dict(null=("obs",)), INVALID),
        (dict(null=("ci",)), INVALID), (dict(null=("cj",)), INVALID), (dict(null=("ci", "cj")), INVALID),
        (dict(H=0), INVALID), (dict(W=0), INVALID), (dict(H=-2), INVALID), (dict(diag=True), INVALID),     # 4 x 5: not square
        (dict(K=0), INVALID), (dict(K=-1), INVALID), (dict(w=-1, small=True), INVALID), (dict(G=0), INVALID), (dict(G=-3), INVALID),
        (dict(offsets=[1, 1, 3]), INVALID), (dict(offsets=[0, 2, 1]), INVALID), (dict(offsets=[0, -1, 3]), INVALID),
        (dict(orient=np.array([0, 4, 0])), INVALID), (dict(orient=np.array([255, 0, 0])), INVALID),
        (dict(K=65, small=True), UNSUPPORTED), (dict(w=65, small=True), UNSUPPORTED),
        (dict(G=17, offsets=[0] * 18, small=True), UNSUPPORTED),
        (dict(diag=True, H=65536, W=65536, small=True), UNSUPPORTED),          # n = 2^31 + 2^15
        (dict(H=46341, W=46341, small=True), UNSUPPORTED),                     # n = 2,147,488,281
        (dict(offsets=[0, 1, 1 << 31]), UNSUPPORTED), (dict(offsets=[0, 1 << 40, 1 << 41]), UNSUPPORTED),
        (dict(ci=np.array([1, big, 3])), UNSUPPORTED), (dict(cj=np.array([-big, 2, 3])), UNSUPPORTED),
        (dict(ci=np.array([1, 2, -(1 << 31)])), UNSUPPORTED),
    ]
    for change, want in cases:
        status, obs = _call(gpu, **dict(ok, **change))
        assert status == want, change
        assert _untouched(obs), change
    # the largest coordinates are no error, and sixteen groups with 64 states and no orient are none either
    status, obs = _call(gpu, **dict(ok, ci=np.array([1, big - 1, 3]), cj=np.array([1, -(big - 1), 3])))
    assert status == 0 and obs[0].sum() > 0
    status, obs = _call(gpu, **dict(ok, K=64, G=16, offsets=[0] * 14 + [1, 3, 3], orient=None))
    assert status == 0 and obs[13].any() and obs[14].any() and not obs[15].any() and not obs[:13].any()


@pytest.mark.parametrize("diag", [True, False])
def test_a_bad_label_inside_a_window_and_outside_every_window(gpu, diag):
    H = W = 40
    good = _map("random", H, W, diag, 5, 9)
    i, j = 30, 35
    at = i * W - i * (i - 1) // 2 + (j - i) if diag else i * W + j
    inside = [(30, 35), (27, 38), (33, 32)] + ([(35, 30), (38, 27)] if diag else [])       # (a diagonal region: the mirror cell too)
    outside = [(5, 5), (26, 35), (30, 39), (-50, 35)] + ([(39, 30), (35, 26)] if diag else [(35, 30), (34, 31)])
    for bad_state in (5, 64, 255):
        labels = good.copy()
        labels[at] = bad_state
        for c in inside:
            ci, cj = np.array([1, c[0]]), np.array([1, c[1]])
            status, obs = _call(gpu, labels, H, W, diag, 5, 3, 1, [0, 2], ci, cj, np.array([0, 1]))
            assert status == INVALID and _untouched(obs), (bad_state, c)
        ci, cj = np.array([c[0] for c in outside]), np.array([c[1] for c in outside])
        orient = np.arange(len(outside)) % 4
        # (the restatement on the good map: no window holds the bad cell, so it counts for nothing)
        want = R.table(good, H, W, diag, 5, 3, 1, [0, len(outside)], ci, cj, orient)
        _check(gpu, labels, H, W, diag, 5, 3, 1, [0, len(outside)], ci, cj, orient, ref=want)


# ---- the Python layer -------------------------------------------------------------------------------------------------------
K_MAP = 6
# one chromosome: two diagonal regions and the off-diagonal region between them; a second chromosome with one region
SHAPES = [(30, 30, 1, 2, 2, 1), (30, 25, 0, 2, 32, 1), (25, 25, 1, 32, 32, 1), (12, 12, 1, 0, 0, 2)]
SEAM = 32                                                     # the first bin of the second diagonal region


def _genome(seed=5):
    rng = np.random.default_rng(seed)
    parts, rows, at = [], [], 0
    for r, (H, W, diag, s1, s2, chrom) in enumerate(SHAPES):
        lab = _map("blocky", H, W, bool(diag), K_MAP, seed + r)
        parts.append(lab)
        rows.append([lab.size, at, at + lab.size, H, W, s1, s2, r, diag, chrom])
        at += lab.size
    return np.concatenate(parts), np.array(rows, dtype=np.int64), rng


def _seam_centres(rng):
    """centres on the seam: their windows take cells from all three regions of chromosome 1 and from the mirror image; a few
    elsewhere, on the other chromosome, outside every region and on a chromosome the map does not hold"""
    c = [[1, SEAM, SEAM, 0, 0], [1, SEAM - 1, SEAM, 0, 1], [1, SEAM, SEAM - 2, 1, 2], [1, SEAM + 1, SEAM - 1, 1, 3],
         [1, SEAM - 3, SEAM + 3, 0, 2], [1, SEAM + 3, SEAM - 3, 2, 0], [1, SEAM, SEAM, 0, 0], [1, 2, 2, 2, 1], [1, 0, 56, 2, 3],
         [1, 56, 0, 1, 0], [2, 3, 9, 0, 3], [2, 11, 0, 2, 1], [1, 500, 500, 0, 0], [7, 3, 3, 1, 0]]
    more = np.stack([np.ones(20, dtype=np.int64), rng.integers(0, 60, 20), rng.integers(0, 60, 20), rng.integers(0, 3, 20),
                     rng.integers(0, 4, 20)], axis=1)
    return np.concatenate([np.array(c, dtype=np.int64), more])


def test_state_pileup_across_the_seam_of_three_regions():
    s, L, rng = _genome()
    c = _seam_centres(rng)
    for w in (0, 2, 5):
        got = pileup.state_pileup(s, L, c, w, K=K_MAP, G=4)
        want = R.state_pileup(s, L, c, w, K_MAP, 4)
        assert got["obs"].dtype == np.int64 and got["obs"].shape == want.shape == (4, 2 * w + 1, 2 * w + 1, K_MAP)
        assert np.array_equal(got["obs"], want), (w, np.argwhere(got["obs"] != want)[:5].tolist())
        assert not got["obs"][3].any() and got["n_centres"].tolist() == np.bincount(c[:, 3], minlength=4).tolist()
        assert got["centres_region"].shape == (4, 4) and int(got["flank"]) == w and int(got["K"]) == K_MAP and int(got["G"]) == 4
    # the first seam centre alone, w = 2: its 25 cells come from all three regions -- and from the mirror image of the third
    one = pileup.state_pileup(s, L, c[:1], 2)
    assert one["obs"].sum() == 25 and one["centres_region"].tolist() == [[1], [2], [1], [0]] and int(one["G"]) == 1
    assert one["obs"].shape[-1] == int(s.max()) + 1
    with pytest.raises(RuntimeError):
        pileup.state_pileup(s, L, c, 2, K=int(s.max()))       # a state >= K inside a window


def _write_inputs(tmp_path):
    import scipy.io
    s, L, _ = _genome()
    path = os.path.join(str(tmp_path), "estimate_ou_7.mat")
    scipy.io.savemat(path, dict(state_vec=s.reshape(1, -1), state_vec_smooth=(K_MAP - 1 - s).reshape(1, -1), len_vec=L))
    bed = os.path.join(str(tmp_path), "sites.bed")
    with open(bed, "w") as fh:
        fh.write("#chrom start stop name score strand\nchr1 1600000 1610000 ctcf 0 +\nchr1 1540000 1560000 ctcf 0 -\n"
                 "chr1 400000 450000 border\nchrX 0 5 ctcf\nchr2 150000 160000 border 0 .\n")
    bedpe = os.path.join(str(tmp_path), "loops.bedpe")
    with open(bedpe, "w") as fh:
        fh.write("chr1 1400000 1450000 chr1 1700000 1750000 loop\nchr1 2000000 2050000 chr1 500000 550000\nchr1 0 5 chr2 0 5 loop\n")
    return s, L, path, bed, bedpe


def test_pileup_files_round_trip(tmp_path):
    s, L, path, bed, _ = _write_inputs(tmp_path)
    out = pileup.pileup_files(path, str(tmp_path / "out"), 50000, field="state_vec_smooth", bed=bed, flank_bp=149999, shift_bp=200000)
    assert os.path.basename(out) == "pileup_estimate_ou_7.npz"
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["pileup_estimate_ou_7.npz", "pileup_estimate_ou_7.txt",
                                                         "pileup_estimate_ou_7_border.png", "pileup_estimate_ou_7_ctcf.png"]
    z = np.load(out, allow_pickle=False)
    anchors = pileup.read_anchors(bed, L, 50000)
    assert anchors["names"] == ["ctcf", "border"] and anchors["skipped_lines"] == 1 and z["names"].tolist() == anchors["names"]
    assert anchors["centres"].tolist() == [[1, 32, 32, 0, 0], [1, 31, 31, 0, 1], [1, 8, 8, 1, 0], [2, 3, 3, 1, 0]]
    ref = R.state_pileup(K_MAP - 1 - s, L, pileup.with_controls(anchors["centres"], 4, 2), 2, K_MAP, 4)
    assert np.array_equal(z["obs"], ref[:2]) and np.array_equal(z["ctl"], ref[2:]) and z["obs"].any() and z["ctl"].any()
    assert np.array_equal(z["log2_ratio"], pileup.log2_ratio(ref[:2], ref[2:]), equal_nan=True)
    assert z["n_centres"].tolist() == [2, 2, 4, 3] and z["centres_region"].shape == (4, 4)       # (the control at bin 3 - 4 is dropped)
    assert (int(z["flank"]), int(z["shift"]), int(z["K"]), int(z["skipped_lines"]), int(z["resolution"])) == (2, 4, K_MAP, 1, 50000)
    assert str(z["pileup_field"]) == "state_vec_smooth" and str(z["anchor_kind"]) == "bed" and np.array_equal(z["len_vec"], L)
    assert (int(z["flank_bp"]), int(z["shift_bp"])) == (149999, 200000)
    lines = open(os.path.join(str(tmp_path / "out"), "pileup_estimate_ou_7.txt")).read().splitlines()
    cells = [ln.split("\t") for ln in lines[1:]]
    assert lines[0].startswith("#name\tu_bp\tv_bp\ttotal\t") and len(cells) == 2 * 25 and all(len(c) == 9 + K_MAP for c in cells)
    for c in cells:
        g, a, b = anchors["names"].index(c[0]), int(c[1]) // 50000 + 2, int(c[2]) // 50000 + 2
        assert [int(x) for x in c[9:]] == ref[g, a, b].tolist() and int(c[3]) == ref[g, a, b].sum() and int(c[7]) == ref[2 + g, a, b].sum()
    from phylo_hmrf_amd.render import PNG_SIGNATURE
    png = open(os.path.join(str(tmp_path / "out"), "pileup_estimate_ou_7_ctcf.png"), "rb").read()
    assert png.startswith(PNG_SIGNATURE) and png[16:24] == (40).to_bytes(4, "big") * 2          # 5 cells of 8 pixels a side


def test_the_command_line_end_to_end(tmp_path):
    import phylo_hmrf as cli
    s, L, path, _, bedpe = _write_inputs(tmp_path)
    out = cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1", "0.5",
                  "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", str(tmp_path / "cli"), quiet="1",
                  pileup=path, pileup_bedpe=bedpe, pileup_flank="100000")
    assert sorted(os.listdir(str(tmp_path / "cli"))) == ["pileup_estimate_ou_7.npz", "pileup_estimate_ou_7.txt",
                                                         "pileup_estimate_ou_7_loop.png", "pileup_estimate_ou_7_pair.png"]
    z = np.load(out, allow_pickle=False)
    pairs = pileup.read_anchor_pairs(bedpe, L, 50000)
    assert pairs["centres"].tolist() == [[1, 28, 34, 0, 0], [1, 10, 40, 1, 0]] and pairs["skipped_lines"] == 1
    assert np.array_equal(z["obs"], R.state_pileup(s, L, pairs["centres"], 2, K_MAP, 2)) and z["obs"].any()
    assert "ctl" not in z.files and int(z["shift"]) == 0 and np.isnan(z["log2_ratio"]).all() and str(z["anchor_kind"]) == "bedpe"
