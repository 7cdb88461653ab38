"""GPU: the image of one state map (phmrf_render_states, phylo_hmrf_amd.render) against the full-matrix restatement of
tests/render_reference.py.  Everything is integer arithmetic: every comparison is exact, byte for byte."""
import ctypes
import os

import numpy as np
import pytest

from tests import render_reference as R

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4
FILL = 0xA5
EXTRA = np.array([255, 0, 255, 0, 0, 0], dtype=np.uint8)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from phylo_hmrf_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    return L, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _palette(K):
    """K colours of the test's own (none of them a reserved colour), so that a wrong state shows in the RGB bytes"""
    k = np.arange(K)
    return np.stack([10 + 3 * k, 250 - 2 * k, (40 + 97 * k) % 251], axis=1).astype(np.uint8)


def _put(dev, x, dtype, offset=0):
    """x on the device, starting `offset` elements into its buffer"""
    import torch
    a = np.zeros(offset + len(x), dtype=dtype)
    a[offset:] = x
    return torch.from_numpy(a).to(dev)[offset:]


def _call(gpu, labels, H, W, diag, K, f, conf=None, mark=None, outline=False, offset=0, palette=None, extra=EXTRA,
          want_planes=True, want_rgb=True, no_labels=False):
    """-> (status, planes u8 [3, h, w], rgb u8 [h, w, 3]); both buffers are filled with FILL before the call"""
    L, dev, st = gpu
    f_eff = max(1, f)
    h, w = -(-H // f_eff), -(-W // f_eff)
    big = h * w > (1 << 24)                                  # (a call that must be refused: no buffers of that size)
    planes = np.full((3, 1, 1) if big else (3, h, w), FILL, dtype=np.uint8)
    rgb = np.full((1, 1, 3) if big else (h, w, 3), FILL, dtype=np.uint8)
    s_t = _put(dev, labels, np.uint8, offset)
    c_t = None if conf is None else _put(dev, conf, np.float32, offset)
    m_t = None if mark is None else _put(dev, mark, np.uint8, offset)
    pal = _palette(max(K, 1)) if palette is None else palette
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    host = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    status = L.phmrf_render_states(None if no_labels else ptr(s_t), ptr(c_t), ptr(m_t), H, W, int(diag), K, f, host(pal),
                                   host(extra), int(outline), host(planes) if want_planes else None,
                                   host(rgb) if want_rgb else None, st)
    return status, planes, rgb


def _check(gpu, labels, H, W, diag, K, f, conf=None, mark=None, outline=False, offset=0, what=""):
    status, planes, rgb = _call(gpu, labels, H, W, diag, K, f, conf, mark, outline, offset)
    assert status == 0, what
    ref = R.render(labels, H, W, diag, K, f, _palette(K), EXTRA[:3], EXTRA[3:], outline, conf, mark)
    for k, name in enumerate(("state", "conf8", "mark8")):
        assert np.array_equal(planes[k], ref[name]), (what, name, np.argwhere(planes[k] != ref[name])[:5].tolist())
    assert np.array_equal(rgb, ref["rgb"]), (what, "rgb", np.argwhere(rgb != ref["rgb"])[:5].tolist())
    if diag:
        assert np.array_equal(rgb, rgb.transpose(1, 0, 2)), what
    return planes, rgb


# ---- maps -------------------------------------------------------------------------------------------------------------------
def _nodes(M, diag):
    M = np.asarray(M)
    return (M[np.triu_indices(M.shape[0])] if diag else M.reshape(-1)).astype(np.uint8)


def _blocky(rng, H, W, K):
    """a piecewise-constant map: constant tiles of 1 - 9 rows by 1 - 9 columns"""
    rows = np.repeat(np.arange(H), rng.integers(1, 10, H))[:H]
    cols = np.repeat(np.arange(W), rng.integers(1, 10, W))[:W]
    return rng.integers(0, K, (H, W))[rows][:, cols]


def _map(kind, H, W, diag, K, seed):
    rng = np.random.default_rng(seed)
    ii, jj = np.indices((H, W))
    if kind == "random":
        M = rng.integers(0, K, (H, W))
    elif kind == "blocky":
        M = _blocky(rng, H, W, K)
    elif kind == "single":
        M = np.full((H, W), K - 1)
    elif kind == "checkerboard":
        M = (ii + jj) % 2 * (K - 1)
    elif kind.startswith("stripe"):
        M = (jj - ii == int(kind[6:])) * (K - 1)
    elif kind == "dominant":
        M = np.where(rng.random((H, W)) < 0.95, 0, rng.integers(1, K, (H, W)))
    else:
        raise ValueError(kind)
    return _nodes(M, diag)


KINDS = ("random", "blocky", "single", "checkerboard", "stripe0", "stripe1", "stripe2", "dominant")


def _conf(rng, n):
    """float32 in [0, 1] with the ends and -0 among them"""
    c = rng.random(n).astype(np.float32)
    c[::7], c[::11], c[::13] = 0.5, 0.0, 1.0
    c[::17] = np.float32(-0.0)
    return c


def _mark(rng, n):
    return (rng.random(n) < 0.02).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)


def _factors(side):
    """1, 2, 3, 7, 64 and one factor that makes the region a single pixel"""
    return sorted(set((1, 2, 3, 7, 64, max(side, 65))))


# ---- the comparison ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, 2, 5, 63, 64, 65, 130])
@pytest.mark.parametrize("diag", [True, False])
def test_square_regions_at_every_factor(gpu, side, diag):
    """random maps at K = 20 with confidences, marks and the outline: 63, 64, 65 and 130 lie around one and two tiles' worth
    of pixels at f = 1 and 2, the factors divide some sides and not others, the largest makes one pixel of the region"""
    rng = np.random.default_rng(side * 2 + diag)
    n = side * (side + 1) // 2 if diag else side * side
    labels = _map("random", side, side, diag, 20, side)
    conf, mark = _conf(rng, n), _mark(rng, n)
    for f in _factors(side):
        if side == 130 and f == 1:                           # (the f = 1 image of this side: once, below, with everything on)
            continue
        with_all = f % 2 == 1
        _check(gpu, labels, side, side, diag, 20, f, conf if with_all or f == 2 else None, mark if with_all else None,
               outline=with_all, what="side %d diag %d f %d" % (side, diag, f))
    if side == 130:
        _check(gpu, labels, side, side, diag, 20, 1, conf, mark, True, what="side 130 diag %d f 1" % diag)


@pytest.mark.parametrize("H,W", [(1, 70), (70, 1), (37, 129)])
def test_offdiagonal_shapes_at_every_factor(gpu, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    labels = _map("blocky", H, W, False, 20, H + W)
    conf, mark = _conf(rng, H * W), _mark(rng, H * W)
    for f in _factors(max(H, W)):
        _check(gpu, labels, H, W, False, 20, f, conf, mark, outline=f != 2, what="%d x %d f %d" % (H, W, f))


@pytest.mark.parametrize("K", [1, 2, 20, 64])
def test_map_kinds_and_numbers_of_states(gpu, K):
    """every kind of map of tests/test_gpu_domains.py on a diagonal block of side 65 (f = 3, 7) and a 37 x 129 block (f = 2),
    with and without confidences, marks and the outline in turn"""
    kinds = KINDS if K >= 2 else ("random", "blocky", "single")
    for t, kind in enumerate(kinds):
        rng = np.random.default_rng(K * 100 + t)
        for H, W, diag, f in ((65, 65, True, 3 if t % 2 else 7), (37, 129, False, 2)):
            n = H * (H + 1) // 2 if diag else H * W
            labels = _map(kind, H, W, diag, K, K + t)
            _check(gpu, labels, H, W, diag, K, f, _conf(rng, n) if t % 2 == 0 else None, _mark(rng, n) if t % 3 == 0 else None,
                   outline=t % 4 < 2, what="K %d %s %d x %d" % (K, kind, H, W))


def test_a_single_marked_node_in_a_corner_pixel(gpu):
    for H, W, diag, f in ((65, 65, True, 7), (37, 129, False, 7)):
        n = H * (H + 1) // 2 if diag else H * W
        labels = _map("blocky", H, W, diag, 5, 3)
        for at in (0, n - 1, (W - 1) if not diag else (H - 1)):          # first node, last node, the end of the first row
            mark = np.zeros(n, dtype=np.uint8)
            mark[at] = 1
            planes, _ = _check(gpu, labels, H, W, diag, 5, f, None, mark, what="mark at %d" % at)
            assert planes[2].sum() == (2 if diag and at == H - 1 else 1)


def test_confidence_ends(gpu):
    """all 0, all 1, all -0: conf8 0, 255, 0 everywhere; and 1 - 2^-24, the largest float32 below 1, stays below 255"""
    labels = _map("blocky", 65, 65, True, 4, 1)
    n = labels.size
    for value, want in ((0.0, 0), (1.0, 255), (-0.0, 0), (np.nextafter(np.float32(1), np.float32(0)), 254)):
        planes, _ = _check(gpu, labels, 65, 65, True, 4, 7, np.full(n, value, dtype=np.float32), what="conf %r" % value)
        assert (planes[1] == want).all()


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_pointers_that_start_inside_their_buffers(gpu, offset):
    rng = np.random.default_rng(offset)
    for H, W, diag, f in ((63, 63, True, 2), (37, 129, False, 3)):
        n = H * (H + 1) // 2 if diag else H * W
        _check(gpu, _map("blocky", H, W, diag, 20, offset), H, W, diag, 20, f, _conf(rng, n), _mark(rng, n), True, offset=offset,
               what="offset %d" % offset)


@pytest.mark.parametrize("side,diag", [(171, False), (225, True)])
def test_more_tiles_than_the_grid_cap(gpu, side, diag):
    """f = 1: the tiles outnumber the workgroups, so every workgroup makes a second trip with its LDS tables left as the first
    trip left them"""
    from phylo_hmrf_amd import render
    per_row = -(-side // render.TILE)
    tiles = render.TILE * per_row * (per_row + 1) // 2 if diag else side * per_row
    assert tiles > render.GRID_CAP
    n = side * (side + 1) // 2 if diag else side * side
    rng = np.random.default_rng(side)
    labels = _map("blocky", side, side, diag, 20, side)
    _check(gpu, labels, side, side, diag, 20, 1, _conf(rng, n), _mark(rng, n), True, what="side %d" % side)


def test_two_calls_give_the_same_bytes(gpu):
    rng = np.random.default_rng(5)
    labels = _map("random", 130, 130, True, 64, 5)
    conf, mark = _conf(rng, labels.size), _mark(rng, labels.size)
    a = _call(gpu, labels, 130, 130, True, 64, 3, conf, mark, True)
    b = _call(gpu, labels, 130, 130, True, 64, 3, conf, mark, True)
    assert a[0] == b[0] == 0
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_either_output_alone_and_neither(gpu):
    rng = np.random.default_rng(6)
    labels = _map("blocky", 37, 129, False, 20, 6)
    conf = _conf(rng, labels.size)
    status, planes, rgb = _call(gpu, labels, 37, 129, False, 20, 3, conf, None, True)
    s1, p1, r1 = _call(gpu, labels, 37, 129, False, 20, 3, conf, None, True, want_rgb=False)
    s2, p2, r2 = _call(gpu, labels, 37, 129, False, 20, 3, conf, None, True, want_planes=False)
    s3, p3, r3 = _call(gpu, labels, 37, 129, False, 20, 3, conf, None, True, want_planes=False, want_rgb=False)
    assert status == s1 == s2 == s3 == 0
    assert np.array_equal(p1, planes) and (r1 == FILL).all()
    assert np.array_equal(r2, rgb) and (p2 == FILL).all()
    assert (p3 == FILL).all() and (r3 == FILL).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _refused(gpu, want, *args, **kw):
    from phylo_hmrf_amd import _lib
    status, planes, rgb = _call(gpu, *args, **kw)
    assert status == want, (status, _lib.load().phmrf_last_error())
    assert (planes == FILL).all() and (rgb == FILL).all()


def test_every_refusal_leaves_the_outputs_alone(gpu):
    labels = _map("blocky", 20, 20, True, 4, 1)
    n = labels.size
    good = np.full(n, 0.5, dtype=np.float32)
    bad = labels.copy()
    bad[n - 1] = 4
    _refused(gpu, INVALID, bad, 20, 20, True, 4, 3)                           # a label >= K
    _refused(gpu, INVALID, bad, 20, 20, True, 4, 3, want_planes=False, want_rgb=False)
    for bits in (0x7fc00000, 0x7f800000, 0xff800000, 0x3f800001, 0xbf000000, 0x80000001):
        conf = good.copy()                                                   # NaN, +inf, -inf, just above 1, -0.5, -denormal
        conf.view(np.uint32)[n // 2] = bits
        _refused(gpu, INVALID, labels, 20, 20, True, 4, 3, conf)
    _refused(gpu, INVALID, labels, 20, 20, True, 4, 0)                        # factor < 1
    _refused(gpu, INVALID, labels, 20, 20, True, 4, -2)
    _refused(gpu, INVALID, labels, 20, 20, True, 0, 3)                        # K outside 1 .. 64
    _refused(gpu, INVALID, labels, 20, 20, True, 65, 3, palette=np.zeros((65, 3), dtype=np.uint8))
    _refused(gpu, INVALID, labels, 20, 10, True, 4, 3)                        # a diagonal block that is not square
    _refused(gpu, INVALID, labels, 0, 20, False, 4, 3)
    _refused(gpu, INVALID, labels, 20, 20, True, 4, 3, no_labels=True)        # NULL pointers
    L, dev, st = gpu
    s_t = _put(dev, labels, np.uint8)
    out = np.full(3 * 49, FILL, dtype=np.uint8)
    pal = _palette(4)
    for palette, extra in ((None, EXTRA), (pal, None)):
        host = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        assert L.phmrf_render_states(ctypes.c_void_p(s_t.data_ptr()), None, None, 20, 20, 1, 4, 3, host(palette), host(extra), 0,
                                     host(out), host(out), st) == INVALID
        assert (out == FILL).all()
    _refused(gpu, UNSUPPORTED, labels, 20, 20, True, 4, 32769)                # a pixel's count could reach 2^31
    _refused(gpu, UNSUPPORTED, labels, 46341, 46341, False, 4, 1)             # h w >= 2^31 - 64, refused before anything is read
    status, _, _ = _call(gpu, labels, 20, 20, True, 4, 32768)                 # the largest factor itself is fine
    assert status == 0


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def _three_regions():
    """two diagonal regions and an off-diagonal one between them: the slices start at nodes 0, 15 and 60"""
    lv = np.array([[15, 0, 15, 5, 5, 0, 0, 0, 1, 1],
                   [45, 15, 60, 5, 9, 0, 5, 1, 0, 1],
                   [21, 60, 81, 6, 6, 3, 3, 2, 1, 2]], dtype=np.int64)
    rng = np.random.default_rng(11)
    s = np.concatenate([_map("blocky", 5, 5, True, 6, 1), _map("random", 5, 9, False, 6, 2), _map("blocky", 6, 6, True, 6, 3)])
    s[0] = 5                                                 # (K = 6 whatever the draws were)
    return s.astype(np.int64), lv, _conf(rng, 81), _mark(rng, 81)


def test_render_states_on_three_regions(gpu):
    from phylo_hmrf_amd import render
    s, lv, conf, mark = _three_regions()
    pal = render.default_palette(6)
    for kw in (dict(factor=2), dict(max_side=3), dict()):
        res = render.render_states(s, lv, conf=conf, mark=mark, outline=True, **kw)
        assert len(res) == 3
        for row, got in zip(lv, res):
            lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
            f = kw.get("factor") or max(1, -(-max(H, W) // kw.get("max_side", 2048)))
            assert got["factor"] == f
            ref = R.render(s[lo:hi], H, W, diag, 6, f, pal, (255, 0, 255), (0, 0, 0), True, conf[lo:hi], mark[lo:hi])
            for name in ("state", "conf8", "mark8", "rgb"):
                assert got[name].dtype == np.uint8 and np.array_equal(got[name], ref[name]), (kw, name)
    own = _palette(7)
    res = render.render_states(s.reshape(1, -1), lv, palette=own, highlight=(1, 2, 3), outline_colour=(9, 8, 7), factor=1)
    ref = R.render(s[15:60], 5, 9, False, 6, 1, own, (1, 2, 3), (9, 8, 7), False)
    assert np.array_equal(res[1]["rgb"], ref["rgb"]) and (res[1]["conf8"] == 255).all() and not res[1]["mark8"].any()
    with pytest.raises(RuntimeError, match="status 1"):
        render.render_states(s, lv, conf=np.full(81, 1.5))


def test_render_files_and_the_mark_of_a_comparison(gpu, tmp_path):
    import scipy.io
    from phylo_hmrf_amd import render
    s, lv, conf, _ = _three_regions()
    smooth = s.copy()
    smooth[15:60] = 2
    path, other = str(tmp_path / "segment_0_6.mat"), str(tmp_path / "compare_a__b.mat")
    scipy.io.savemat(path, dict(state_vec=s.reshape(1, -1), state_vec_smooth=smooth.reshape(1, -1), len_vec=lv, conf=conf))
    diff = np.zeros(81, dtype=np.uint8)
    diff[[3, 20, 21, 80]] = 2
    diff[[4, 40]] = 1                                        # differs below min_conf: not a differential domain's bin pair
    scipy.io.savemat(other, dict(diff_vec=diff.reshape(1, -1), len_vec=lv))
    colours = str(tmp_path / "colours.txt")
    own = _palette(8)
    with open(colours, "w") as fh:
        fh.write("".join("%d\t%d\t%d\n" % tuple(c) for c in own))
    out_dir = str(tmp_path / "out")
    out = render.render_files(path, out_dir, max_side=4, palette_path=colours, outline=True, use_conf=True, mark_path=other)
    assert out == os.path.join(out_dir, "render_segment_0_6.npz")
    z = np.load(out, allow_pickle=False)
    assert z["factor"].tolist() == [2, 3, 2] and np.array_equal(z["palette"], own[:6]) and np.array_equal(z["len_vec"], lv)
    assert str(z["render_field"]) == "state_vec" and int(z["render_side"]) == 4 and int(z["render_outline"]) == 1
    assert int(z["render_conf"]) == 1 and str(z["render_mark"]) == "compare_a__b.mat"
    names = sorted(f for f in os.listdir(out_dir))
    assert names == ["render_segment_0_6.npz", "render_segment_0_6_legend.txt", "render_segment_0_6_r0_chr1.png",
                     "render_segment_0_6_r1_chr1.png", "render_segment_0_6_r2_chr2.png"]
    for r, row in enumerate(lv):
        lo, hi, H, W, diag = (int(row[k]) for k in (1, 2, 3, 4, 8))
        ref = R.render(s[lo:hi], H, W, diag, 6, int(z["factor"][r]), own, (255, 0, 255), (0, 0, 0), True, conf[lo:hi],
                       diff[lo:hi] == 2)
        png = R.decode_png(os.path.join(out_dir, "render_segment_0_6_r%d_chr%d.png" % (r, row[9])))
        assert np.array_equal(png, ref["rgb"])
        for name in ("state", "conf8", "mark8"):
            assert np.array_equal(z["%s_%d" % (name, r)], ref[name])
        assert ref["mark8"].any()                            # (every region has a highlighted pixel, and only where the reference has)
        assert np.array_equal((png == (255, 0, 255)).all(axis=2), ref["mark8"] == 1)
    legend = open(os.path.join(out_dir, "render_segment_0_6_legend.txt")).read().splitlines()
    assert legend == ["%d\t%d\t%d\t%d" % (k + 1, own[k, 0], own[k, 1], own[k, 2]) for k in range(6)]
    out = render.render_files(path, str(tmp_path / "smooth"), field="state_vec_smooth")
    z = np.load(out, allow_pickle=False)
    assert z["factor"].tolist() == [1, 1, 1] and (z["state_1"] == 2).all() and (z["conf8_1"] == 255).all()
    assert np.array_equal(z["palette"], render.default_palette(6))


def test_the_command_line_draws(gpu, tmp_path):
    import scipy.io
    import phylo_hmrf as cli
    s, lv, _, _ = _three_regions()
    path = str(tmp_path / "estimate_ou_1.mat")
    scipy.io.savemat(path, dict(state_vec=s.reshape(1, -1), len_vec=lv))
    o = cli.parse_args(["--render", path, "--render_side", "3", "--output", str(tmp_path / "img")])
    out = cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                  "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", o.output, quiet="1",
                  render=o.render, render_side=o.render_side)
    assert np.load(out, allow_pickle=False)["factor"].tolist() == [2, 3, 2]
    with pytest.raises(ValueError, match="conf"):
        cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", o.output, quiet="1",
                render=o.render, render_conf="1")
