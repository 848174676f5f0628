"""numpy restatement of DESIGN.md §4g steps 1-3: the (Y, Cb, Cr) triples the colour preview's encoder is given, from the bytes of
a raw frame — orientation, chroma pairing of the 4:2:2 formats, colour conversion, nearest-neighbour scale, overlay.  `triples`
is the contract's index arithmetic as plain loops over the preview's pixels; `triples_vec` is the vectorised form the host test
checks against the loops and the GPU tests use."""
import numpy as np

import np_jpeg_enc as E
import np_jpeg_enc_color as EC
import raw_format_ref as R

FAMILIES = ("YUYV", "UYVY", "RGB3", "BGR3", "RGBA", "BGRA")
# byte of Y inside a pixel's two bytes, bytes of U and V inside its pair's four
YUV422 = {"YUYV": (0, 1, 3), "YUY2": (0, 1, 3), "UYVY": (1, 0, 2)}


def source_triple(row, fourcc, x):
    """(c0, c1, c2) of pixel x of one source row (a flat uint8 array that starts at the row's first byte)."""
    if fourcc in YUV422:
        yo, uo, vo = YUV422[fourcc]
        pair = 4 * (x >> 1)
        return int(row[2 * x + yo]), int(row[pair + uo]), int(row[pair + vo])
    bpp, ri, gi, bi = R.RGB_ORDER[fourcc]
    y, cb, cr = EC.ycc(row[bpp * x + ri], row[bpp * x + gi], row[bpp * x + bi])
    return int(y), int(cb), int(cr)


def triples(buf, fourcc, sw, sh, stride, o, pw, ph, dets=None):
    """P [ph][pw][3] as loops: for every preview pixel its pixel of the oriented frame O (scale), O's pixel of the source S (the
    four index maps of §4d), the triple there, then the overlay."""
    o = R.ORIENT_CODE[o] if isinstance(o, str) else o
    b = np.asarray(buf, np.uint8).reshape(-1)
    W, H = (sh, sw) if o in (1, 3) else (sw, sh)
    mask = E.overlay_mask(dets, pw, ph, W, H) if dets is not None else None
    P = np.zeros((ph, pw, 3), np.uint8)
    for y in range(ph):
        oy = ((2 * y + 1) * H) // (2 * ph)
        for x in range(pw):
            ox = ((2 * x + 1) * W) // (2 * pw)
            if o == 0:
                sy, sx = oy, ox
            elif o == 1:
                sy, sx = sh - 1 - ox, oy
            elif o == 2:
                sy, sx = sh - 1 - oy, sw - 1 - ox
            else:
                sy, sx = ox, sw - 1 - oy
            P[y, x] = source_triple(b[sy * stride:], fourcc, sx)
            if mask is not None and mask[y, x]:
                P[y, x] = EC.ycc(0, 255, 0)
    return P


def source_vec(buf, fourcc, sw, sh, stride):
    """S [sh][sw][3]: the triples of every source pixel."""
    b = np.asarray(buf, np.uint8).reshape(-1)
    ms = R.min_stride(fourcc, sw)
    rows = np.lib.stride_tricks.as_strided(b[:(sh - 1) * stride + ms], (sh, ms), (stride, 1))
    if fourcc in YUV422:
        yo, uo, vo = YUV422[fourcc]
        pair = 4 * (np.arange(sw) >> 1)
        return np.stack([rows[:, 2 * np.arange(sw) + yo], rows[:, pair + uo], rows[:, pair + vo]], -1)
    bpp, ri, gi, bi = R.RGB_ORDER[fourcc]
    px = rows[:, :bpp * sw].reshape(sh, sw, bpp)
    return np.stack(EC.ycc(px[:, :, ri], px[:, :, gi], px[:, :, bi]), -1)


def triples_vec(buf, fourcc, sw, sh, stride, o, pw, ph, dets=None):
    o = R.ORIENT_CODE[o] if isinstance(o, str) else o
    S = source_vec(buf, fourcc, sw, sh, stride)
    O = (S, np.rot90(S, -1), S[::-1, ::-1], np.rot90(S, 1))[o]
    H, W = O.shape[:2]
    sy = ((2 * np.arange(ph, dtype=np.int64) + 1) * H) // (2 * ph)
    sx = ((2 * np.arange(pw, dtype=np.int64) + 1) * W) // (2 * pw)
    P = np.ascontiguousarray(O[sy][:, sx])
    if dets is not None:
        P[E.overlay_mask(dets, pw, ph, W, H)] = EC.OVERLAY_TRIPLE
    return P


def pack_colour(rng, fourcc, sw, sh, stride=None, pad_byte=0xA7):
    """A random source frame [sh][stride] of a packed colour family: every byte of a row's first min_stride random (luma, chroma,
    alpha alike), pad_byte behind them."""
    ms = R.min_stride(fourcc, sw)
    stride = ms if stride is None else stride
    buf = np.full((sh, stride), pad_byte, np.uint8)
    buf[:, :ms] = rng.integers(0, 256, (sh, ms), dtype=np.uint8)
    return buf
