"""The image of a state map restated on the region's full matrix in NumPy and Python integers (the
definition the GPU's phmrf_render_states is held to), and the tests' own PNG decoder.  Host only, shares nothing with
phylo_hmrf_amd.render."""
import struct
import zlib

import numpy as np

ONE = 1 << 24                    # the fixed point of the confidence sums


def full(values, H, W, diag):
    """node order -> the H x W matrix: a diagonal block's upper triangle mirrored"""
    values = np.asarray(values)
    if not diag:
        return values.reshape(H, W).copy()
    M = np.zeros((H, H), dtype=values.dtype)
    iu = np.triu_indices(H)
    M[iu] = values
    M.T[iu] = values
    return M


def planes(labels, H, W, diag, K, f, conf=None, mark=None):
    """-> (state, conf8, mark8) u8 [h, w]"""
    M = full(np.asarray(labels).astype(np.int64), H, W, diag)
    C = None if conf is None else full(np.asarray(conf, dtype=np.float32), H, W, diag)
    B = None if mark is None else full(np.asarray(mark), H, W, diag)
    h, w = -(-H // f), -(-W // f)
    state = np.zeros((h, w), dtype=np.uint8)
    conf8 = np.full((h, w), 255, dtype=np.uint8)
    mark8 = np.zeros((h, w), dtype=np.uint8)
    for p in range(h):
        for q in range(w):
            rows, cols = slice(p * f, min(H, (p + 1) * f)), slice(q * f, min(W, (q + 1) * f))
            cells = M[rows, cols].reshape(-1)
            counts = np.bincount(cells, minlength=K)
            s = int(np.argmax(counts))                       # (the first of equal counts: the lowest state)
            state[p, q] = s
            if C is not None:
                c = C[rows, cols].reshape(-1)[cells == s]
                total = sum(int(np.floor(np.float64(x) * ONE)) for x in c)     # (-0.0 -> 0)
                conf8[p, q] = (255 * total) // (int(counts[s]) * ONE)
            if B is not None:
                mark8[p, q] = 1 if np.any(B[rows, cols] != 0) else 0
    return state, conf8, mark8


def colour(state, conf8, mark8, palette, highlight, outline_colour, outline):
    """-> rgb u8 [h, w, 3]"""
    s = np.asarray(state).astype(np.int64)
    t = 64 + (191 * np.asarray(conf8).astype(np.int64)) // 255
    rgb = 255 - ((255 - np.asarray(palette).astype(np.int64)[s]) * t[:, :, None]) // 255
    if outline:
        edge = np.zeros(s.shape, dtype=bool)
        edge[:, :-1] |= s[:, :-1] != s[:, 1:]                # the pixel to the right
        edge[:-1, :] |= s[:-1, :] != s[1:, :]                # the pixel below
        rgb[edge] = np.asarray(outline_colour, dtype=np.int64)
    rgb[np.asarray(mark8) != 0] = np.asarray(highlight, dtype=np.int64)
    return rgb.astype(np.uint8)


def render(labels, H, W, diag, K, f, palette, highlight=(255, 0, 255), outline_colour=(0, 0, 0), outline=False, conf=None,
           mark=None):
    """-> dict(state, conf8, mark8, rgb)"""
    state, conf8, mark8 = planes(labels, H, W, diag, K, f, conf, mark)
    return dict(state=state, conf8=conf8, mark8=mark8,
                rgb=colour(state, conf8, mark8, palette, highlight, outline_colour, outline))


def decode_png(path):
    """-> u8 [h, w, 3] of an 8-bit RGB PNG without interlace whose scanlines all have filter type 0; every CRC is checked"""
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(blob):
        (size,) = struct.unpack(">I", blob[at:at + 4])
        kind, data = blob[at + 4:at + 8], blob[at + 8:at + 8 + size]
        (crc,) = struct.unpack(">I", blob[at + 8 + size:at + 12 + size])
        assert crc == zlib.crc32(kind + data) & 0xffffffff, kind
        chunks.append((kind, data))
        at += 12 + size
    assert at == len(blob)
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    assert len(chunks[0][1]) == 13
    w, h, depth, colour_type, compression, filtering, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour_type, compression, filtering, interlace) == (8, 2, 0, 0, 0)
    assert all(kind in (b"IHDR", b"IDAT", b"IEND") for kind, _ in chunks)
    raw = zlib.decompress(b"".join(data for kind, data in chunks if kind == b"IDAT"))
    assert len(raw) == h * (1 + 3 * w)
    lines = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not lines[:, 0].any()                             # filter type 0 on every scanline
    return lines[:, 1:].reshape(h, w, 3).copy()
