"""Images of a state map: what the reference's color_map_sub.m / color_map_test.m / color_map2.m draw.

`render_states(state_vec, len_vec, ...)` reduces, region by region, the region's full matrix by an integer factor on the GPU
(phmrf_render_states, csrc/render.hip): a pixel takes the state most of its bin pairs hold, fades towards white with the
mean confidence of those bin pairs, and is highlighted when one of its bin pairs is marked.  `write_png(path, rgb)` writes an
image with the standard library alone, `render_files(...)` is the command line's --render FILE.mat.

Everything the GPU computes here is integer arithmetic: two runs give the same bytes.  There is no host fallback.

len_vec rows: [n, start, stop, H, W, start_bin1, start_bin2, region_id, type (1 = diagonal), chrom].
"""
import ctypes
import os
import struct
import zlib

import numpy as np

from .maps import MAX_STATES, check_len_vec, check_state_vec, conf_array, device, load_map, regions, stem

GRID_CAP = 1024                  # csrc/render.hip RENDER_GRID_CAP: workgroups (of 256 lanes) of its kernels
TILE = 32                        # csrc/render.hip RENDER_TILE: consecutive pixels of one pixel row a workgroup votes at a time
MAX_FACTOR = 32768               # csrc/render.hip RENDER_MAX_FACTOR
HIGHLIGHT = (255, 0, 255)
OUTLINE = (0, 0, 0)
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def choose_factor(H, W, max_side):
    """-> the smallest integer factor at which neither side of an H x W region exceeds max_side pixels"""
    H, W, max_side = int(H), int(W), int(max_side)
    if H < 1 or W < 1 or max_side < 1:
        raise ValueError("H, W and max_side must be >= 1")
    return max(1, -(-max(H, W) // max_side))


def default_palette(K):
    """-> u8 [K, 3], K <= 64: the hues 137 k mod 360 degrees (all different: 137 and 360 share no factor) at three
    brightnesses in turn, by integer HSV arithmetic with the smallest channel at 30.  The colours are pairwise distinct; the
    largest channel is at most 225 and the smallest 30, so none is white, black or the default highlight."""
    K = int(K)
    if K < 1 or K > MAX_STATES:
        raise ValueError("K must be in 1 .. %d" % MAX_STATES)
    out = np.zeros((K, 3), dtype=np.uint8)
    low = 30
    for k in range(K):
        top = (225, 165, 195)[k % 3]
        sector, frac = divmod((137 * k) % 360, 60)
        up = low + (top - low) * frac // 60
        down = top - (top - low) * frac // 60
        out[k] = ((top, up, low), (down, top, low), (low, top, up), (low, down, top), (up, low, top), (top, low, down))[sector]
    return out


def _palette(palette, K):
    if palette is None:
        return default_palette(K)
    p = np.asarray(palette)
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < K or p.dtype.kind not in "iu" or (p.size and (p.min() < 0 or p.max() > 255)):
        raise ValueError("a palette holds at least K = %d rows of three integers in 0 .. 255" % K)
    return np.ascontiguousarray(p[:K].astype(np.uint8))


def _colour(c, what):
    a = np.asarray(c)
    if a.shape != (3,) or a.dtype.kind not in "iu" or a.min() < 0 or a.max() > 255:
        raise ValueError("%s must be three integers in 0 .. 255" % what)
    return a.astype(np.uint8)


def load_palette(path, K):
    """-> u8 [K, 3] from a text file of `R G B` rows (whitespace separated integers in 0 .. 255, at least K rows; blank lines
    are skipped): the format of the reference's processing/color_vec.txt"""
    K = int(K)
    if K < 1 or K > MAX_STATES:
        raise ValueError("K must be in 1 .. %d" % MAX_STATES)
    rows = []
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 3 or not all(x.isdigit() for x in parts) or any(int(x) > 255 for x in parts):
                raise ValueError("%s line %d: expected three integers in 0 .. 255, got %r" % (path, number, line.strip()))
            rows.append([int(x) for x in parts])
    if len(rows) < K:
        raise ValueError("%s holds %d colours for %d states" % (path, len(rows), K))
    return np.array(rows[:K], dtype=np.uint8)


def render_states(state_vec, len_vec, conf=None, mark=None, max_side=2048, factor=None, palette=None, outline=False,
                  highlight=HIGHLIGHT, outline_colour=OUTLINE):
    """Region by region -> a list of dicts:
      rgb u8 [h, w, 3]                   the image, row 0 at the top (h = ceil(H / factor), w = ceil(W / factor))
      state, conf8, mark8 u8 [h, w]      the winning state, its mean confidence in 0 .. 255 (255 without conf), marked or not
      factor                             the region's reduction: `factor`, or choose_factor(H, W, max_side)
    conf float32 [n] in [0, 1] shades, mark [n] (non-zero: marked) highlights; palette u8 [>= K, 3] (None: default_palette)."""
    import torch
    from . import _lib
    s = check_state_vec(state_vec)
    L = check_len_vec(len_vec, s.shape[0])
    n = s.shape[0]
    if factor is not None and int(factor) < 1:
        raise ValueError("factor must be >= 1")
    if factor is None and int(max_side) < 1:
        raise ValueError("max_side must be >= 1")
    K = int(s.max()) + 1 if n else 1
    pal = _palette(palette, K)
    extra = np.concatenate([_colour(highlight, "highlight"), _colour(outline_colour, "outline_colour")])
    conf = None if conf is None else conf_array(conf, n, "conf")
    if mark is not None:
        mark = np.ascontiguousarray(np.asarray(mark).reshape(-1) != 0).astype(np.uint8)
        if mark.shape[0] != n:
            raise ValueError("mark has %d entries for %d nodes" % (mark.shape[0], n))
    lib, dev, stream = device()
    s_t = torch.from_numpy(s.astype(np.uint8)).to(dev)
    c_t = None if conf is None else torch.from_numpy(conf).to(dev)
    m_t = None if mark is None else torch.from_numpy(mark).to(dev)
    null = ctypes.c_void_p(None)
    out = []
    for _, lo, hi, H, W, diag, _ in regions(L):
        f = choose_factor(H, W, max_side) if factor is None else int(factor)
        h, w = -(-H // f), -(-W // f)
        planes = np.zeros((3, h, w), dtype=np.uint8)
        rgb = np.zeros((h, w, 3), dtype=np.uint8)
        _lib.check(lib.phmrf_render_states(
            ctypes.c_void_p(s_t[lo:hi].data_ptr()), null if c_t is None else ctypes.c_void_p(c_t[lo:hi].data_ptr()),
            null if m_t is None else ctypes.c_void_p(m_t[lo:hi].data_ptr()), H, W, diag, K, f,
            pal.ctypes.data_as(ctypes.c_void_p), extra.ctypes.data_as(ctypes.c_void_p), int(bool(outline)),
            planes.ctypes.data_as(ctypes.c_void_p), rgb.ctypes.data_as(ctypes.c_void_p), stream))
        out.append(dict(rgb=rgb, state=planes[0], conf8=planes[1], mark8=planes[2], factor=f))
    return out


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def write_png(path, rgb):
    """rgb u8 [h, w, 3] -> an 8-bit RGB PNG: one IDAT, filter type 0 on every scanline.  Standard library only."""
    a = np.asarray(rgb)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png takes a u8 array [h, w, 3] with h, w >= 1 (got %s %s)" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    lines = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    lines[:, 1:] = a.reshape(h, 3 * w)
    with open(path, "wb") as fh:
        fh.write(PNG_SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                 + _chunk(b"IDAT", zlib.compress(lines.tobytes(), 6)) + _chunk(b"IEND", b""))


def load_mark(path, len_vec):
    """-> u8 [n]: 1 at the bin pairs of the differential domains (diff_vec == 2) of a compare_*.mat on the same regions"""
    import scipy.io
    d = scipy.io.loadmat(path)
    if "diff_vec" not in d or "len_vec" not in d:
        raise ValueError("%s holds no diff_vec / len_vec: --render_mark takes a compare_*.mat" % path)
    diff = np.asarray(d["diff_vec"]).reshape(-1)
    theirs = check_len_vec(d["len_vec"], diff.shape[0])
    if theirs.shape[0] != len_vec.shape[0] or not np.array_equal(theirs[:, :10], len_vec[:, :10]):
        raise ValueError("%s does not hold the regions of the map (len_vec columns 0 - 9 differ)" % path)
    return (diff == 2).astype(np.uint8)


def render_files(path, output_path, field="state_vec", max_side=2048, palette_path="", outline=False, use_conf=False,
                 mark_path=""):
    """The command line's --render: draw the `field` of one estimate_ou_*.mat / segment_*.mat / smooth_*.mat.  Writes under
    output_path one render_<stem>_r<region>_chr<chrom>.png per region (region: the row of len_vec), render_<stem>.npz (the
    planes state_<r>, conf8_<r>, mark8_<r>, and factor, palette, len_vec and the settings; no pickles) and
    render_<stem>_legend.txt (per state: state + 1, R, G, B).  -> the .npz"""
    if int(max_side) < 1:
        raise ValueError("max_side must be >= 1")
    s, L, conf = load_map(path, field)
    if use_conf and conf is None:
        raise ValueError("%s holds no conf to shade by (--render_conf 1 takes a segment_*.mat)" % path)
    K = int(s.max()) + 1 if s.size else 1
    palette = load_palette(palette_path, K) if palette_path else default_palette(K)
    mark = load_mark(mark_path, L) if mark_path else None
    res = render_states(s, L, conf=conf if use_conf else None, mark=mark, max_side=int(max_side), palette=palette,
                        outline=bool(outline))
    os.makedirs(output_path, exist_ok=True)
    base = stem(path)
    arrays = dict(factor=np.array([r["factor"] for r in res], dtype=np.int64), palette=palette, len_vec=L,
                  render_field=np.array(field), render_side=np.int64(max_side), render_outline=np.int64(bool(outline)),
                  render_conf=np.int64(bool(use_conf)), render_mark=np.array(os.path.basename(mark_path)),
                  highlight=np.array(HIGHLIGHT, dtype=np.uint8), outline_colour=np.array(OUTLINE, dtype=np.uint8))
    for r, (row, img) in enumerate(zip(L, res)):
        write_png(os.path.join(output_path, "render_%s_r%d_chr%d.png" % (base, r, int(row[9]))), img["rgb"])
        for name in ("state", "conf8", "mark8"):
            arrays["%s_%d" % (name, r)] = img[name]
    out = os.path.join(output_path, "render_%s.npz" % base)
    np.savez(out, **arrays)
    with open(os.path.join(output_path, "render_%s_legend.txt" % base), "w") as fh:
        for k in range(K):
            fh.write("%d\t%d\t%d\t%d\n" % (k + 1, palette[k, 0], palette[k, 1], palette[k, 2]))
    return out
