"""numpy restatement of DESIGN.md §4s: the planar 4:2:0 raw formats with their chroma planes (NV12, NV21, I420, YV12 with
CK_RAW_PLANES).  `pack_planes` lays three arrays out as the contract words it; `triples` is the contract's index arithmetic as plain
loops, `triples_vec` its vectorised form (the host test checks one against the other, the GPU tests use the second); `yuyv_twin` is
the YUYV frame whose triples are the same, which ties the new source kind to the 4:2:2 one that was there before it.  A helper, not
a test."""
import numpy as np

import np_jpeg_enc as E
import np_jpeg_enc_color as EC
import raw_format_ref as R

FOURCCS = ("NV12", "NV21", "I420", "YV12")
INTERLEAVED = ("NV12", "NV21")
CB_FIRST = ("NV12", "I420")
CK_RAW_PLANES = 0x100


def chroma_size(sw, sh):
    return (sw + 1) // 2, (sh + 1) // 2


def min_stride(sw):
    return 2 * ((sw + 1) // 2)


def formulas(fourcc, sw, sh, stride):
    """(offset[3], row_stride[3], step[3], bytes) of Y, Cb, Cr by the contract's words."""
    cw, ch = chroma_size(sw, sh)
    base = stride * sh
    if fourcc in INTERLEAVED:
        first, second, rs, st = base, base + 1, stride, 2
    else:
        assert stride % 2 == 0
        first, second, rs, st = base, base + (stride // 2) * ch, stride // 2, 1
    cb, cr = (first, second) if fourcc in CB_FIRST else (second, first)
    return (0, cb, cr), (stride, rs, rs), (1, st, st), stride * (sh + ch)


def random_planes(rng, sw, sh):
    """Y [sh][sw] anything, Cb [ch][cw] in 0..127, Cr [ch][cw] in 128..255: a swapped order shows in every sample."""
    cw, ch = chroma_size(sw, sh)
    return (rng.integers(0, 256, (sh, sw), dtype=np.uint8), rng.integers(0, 128, (ch, cw), dtype=np.uint8),
            rng.integers(128, 256, (ch, cw), dtype=np.uint8))


def pack_planes(y, cb, cr, fourcc, stride=None, pad_byte=0xA7, seed=0):
    """The frame [sh + ch][stride] (one buffer of stride * (sh + ch) bytes).  Bytes no plane holds are pad_byte, or random bytes
    drawn from `seed` when pad_byte is None."""
    y, cb, cr = (np.asarray(a, np.uint8) for a in (y, cb, cr))
    sh, sw = y.shape
    cw, ch = chroma_size(sw, sh)
    assert cb.shape == (ch, cw) and cr.shape == (ch, cw)
    stride = min_stride(sw) if stride is None else stride
    assert stride >= min_stride(sw)
    n = stride * (sh + ch)
    flat = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8) if pad_byte is None else np.full(n, pad_byte, np.uint8)
    off, rs, st, total = formulas(fourcc, sw, sh, stride)
    assert total == n
    for j in range(sh):
        flat[j * stride:j * stride + sw] = y[j]
    for plane, c in ((cb, 1), (cr, 2)):
        for j in range(ch):
            a = off[c] + j * rs[c]
            flat[a:a + st[c] * cw:st[c]] = plane[j]
    return flat.reshape(sh + ch, stride)


def source_xy(o, sw, sh, ox, oy):
    """The source pixel behind pixel (ox, oy) of the oriented frame: the four index maps of §4d."""
    if o == 0:
        return ox, oy
    if o == 1:
        return oy, sh - 1 - ox
    if o == 2:
        return sw - 1 - ox, sh - 1 - oy
    return sw - 1 - oy, ox


def triples(buf, fourcc, sw, sh, stride, orientation):
    """O [H][W][3] as loops: Y = luma[y][x], Cb = Cb[y >> 1][x >> 1], Cr = Cr[y >> 1][x >> 1] of the source pixel."""
    o = R.ORIENT_CODE[orientation] if isinstance(orientation, str) else orientation
    b = np.asarray(buf, np.uint8).reshape(-1)
    off, rs, st, _ = formulas(fourcc, sw, sh, stride)
    W, H = (sh, sw) if o in (1, 3) else (sw, sh)
    O = np.zeros((H, W, 3), np.uint8)
    for oy in range(H):
        for ox in range(W):
            x, y = source_xy(o, sw, sh, ox, oy)
            O[oy, ox] = (b[y * stride + x], b[off[1] + (y >> 1) * rs[1] + (x >> 1) * st[1]], b[off[2] + (y >> 1) * rs[2] + (x >> 1) * st[2]])
    return O


def source_vec(buf, fourcc, sw, sh, stride):
    """S [sh][sw][3]: the triples of every source pixel."""
    b = np.asarray(buf, np.uint8).reshape(-1)
    off, rs, st, _ = formulas(fourcc, sw, sh, stride)
    yy, xx = np.mgrid[0:sh, 0:sw]
    return np.stack([b[yy * stride + xx], b[off[1] + (yy >> 1) * rs[1] + (xx >> 1) * st[1]], b[off[2] + (yy >> 1) * rs[2] + (xx >> 1) * st[2]]], -1)


def triples_vec(buf, fourcc, sw, sh, stride, orientation):
    o = R.ORIENT_CODE[orientation] if isinstance(orientation, str) else orientation
    S = source_vec(buf, fourcc, sw, sh, stride)
    return np.ascontiguousarray((S, np.rot90(S, -1), S[::-1, ::-1], np.rot90(S, 1))[o])


def preview(O, pw, ph, dets=None):
    """§4g's scale rule and overlay on the oriented triples O [H][W][3]: P [ph][pw][3]."""
    H, W = O.shape[:2]
    sy = ((2 * np.arange(ph, dtype=np.int64) + 1) * H) // (2 * ph)
    sx = ((2 * np.arange(pw, dtype=np.int64) + 1) * W) // (2 * pw)
    P = np.ascontiguousarray(O[sy][:, sx])
    if dets is not None:
        P[E.overlay_mask(dets, pw, ph, W, H)] = EC.OVERLAY_TRIPLE
    return P


def yuyv_twin(buf, fourcc, sw, sh, stride):
    """The YUYV frame [sh][4 ceil(sw / 2)] of the same sw x sh with the same triples: pair x >> 1 of row y carries
    Cb[y >> 1][x >> 1] and Cr[y >> 1][x >> 1].  (The luma byte of a pair's missing second pixel, for odd sw, is 0.)"""
    S = source_vec(buf, fourcc, sw, sh, stride)
    cw = (sw + 1) // 2
    out = np.zeros((sh, 4 * cw), np.uint8)
    out[:, 0:2 * sw:2] = S[:, :, 0]
    out[:, 1::4] = S[:, 0::2, 1]
    out[:, 3::4] = S[:, 0::2, 2]
    return out
