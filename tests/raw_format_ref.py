"""numpy restatement of DESIGN.md §4d: raw camera formats -> luma -> orientation.  Line by line the contract's index arithmetic
(`luma`, `orient`: plain loops), each with a second, vectorised form that the host test checks against the loops and the GPU
tests use at full size.  `pack` builds source buffers whose chroma, alpha and padding bytes are unlike the luma."""
import numpy as np

LUMA_FIRST = ("GREY", "GRAY", "Y800", "NV12", "NV21", "I420", "YV12")
PLANAR_420 = ("NV12", "NV21", "I420", "YV12")
YUV422 = {"YUYV": 0, "YUY2": 0, "UYVY": 1}                       # byte of the luma inside a pixel's two bytes
RGB_ORDER = {"RGB3": (3, 0, 1, 2), "RGB ": (3, 0, 1, 2), "BGR3": (3, 2, 1, 0), "BGR ": (3, 2, 1, 0),
             "RGBA": (4, 0, 1, 2), "BGRA": (4, 2, 1, 0)}          # bytes per pixel, position of R, G, B
FOURCCS = LUMA_FIRST + tuple(YUV422) + tuple(RGB_ORDER)
# one fourcc per family (two fourccs of a family are the same bytes under another name)
FAMILIES = ("GREY", "NV12", "YUYV", "UYVY", "RGB3", "BGR3", "RGBA", "BGRA")
ORIENTATIONS = ("none", "clockwise", "rotate-180", "counterclockwise")
ORIENT_CODE = {name: i for i, name in enumerate(ORIENTATIONS)}


def L(r, g, b):
    """(19595 R + 38470 G + 7471 B + 32768) >> 16 in unsigned 32-bit arithmetic."""
    r, g, b = (np.asarray(v).astype(np.uint32) for v in (r, g, b))
    return ((np.uint32(19595) * r + np.uint32(38470) * g + np.uint32(7471) * b + np.uint32(32768)) >> np.uint32(16)).astype(np.uint8)


def is_colour(fourcc):
    return fourcc in RGB_ORDER


def source_size(w, h, orientation):
    """(sw, sh) of the source of an oriented w x h frame."""
    return (h, w) if ORIENT_CODE[orientation] in (1, 3) else (w, h)


def min_stride(fourcc, sw):
    if fourcc in LUMA_FIRST:
        return sw
    if fourcc in YUV422:
        return 4 * ((sw + 1) // 2)
    if fourcc in RGB_ORDER:
        return RGB_ORDER[fourcc][0] * sw
    raise KeyError(fourcc)


def pack(image, fourcc, stride=None, pad_byte=0xA7, seed=0):
    """A source buffer [rows][stride] for `image`: a luma image [sh][sw] for the luma-first and 4:2:2 formats (chroma: random bytes),
    an RGB image [sh][sw][3] for the colour formats (alpha: random bytes).  Bytes of a row past the minimum stride are pad_byte;
    the 4:2:0 formats get their chroma rows behind the luma plane."""
    rng = np.random.default_rng(seed)
    image = np.asarray(image, np.uint8)
    sh, sw = image.shape[:2]
    ms = min_stride(fourcc, sw)
    stride = ms if stride is None else stride
    assert stride >= ms
    rows = sh + (sh + 1) // 2 if fourcc in PLANAR_420 else sh
    buf = np.full((rows, stride), pad_byte, np.uint8)
    if fourcc in LUMA_FIRST:
        buf[:sh, :sw] = image
        if rows > sh:
            buf[sh:, :sw] = rng.integers(0, 256, (rows - sh, sw), dtype=np.uint8)
    elif fourcc in YUV422:
        yo = YUV422[fourcc]
        buf[:, :ms] = rng.integers(0, 256, (sh, ms), dtype=np.uint8)   # chroma everywhere, luma over it
        buf[:, yo:2 * sw:2] = image
    else:
        bpp, ri, gi, bi = RGB_ORDER[fourcc]
        px = rng.integers(0, 256, (sh, sw, bpp), dtype=np.uint8)       # (alpha, where there is one)
        px[:, :, ri], px[:, :, gi], px[:, :, bi] = image[:, :, 0], image[:, :, 1], image[:, :, 2]
        buf[:, :ms] = px.reshape(sh, ms)
    return buf


def luma(buf, fourcc, sw, sh, stride):
    """S[sh][sw] from the bytes `buf` (flat), the contract's table as loops."""
    b = np.asarray(buf, np.uint8).reshape(-1)
    S = np.zeros((sh, sw), np.uint8)
    for y in range(sh):
        r = b[y * stride:]
        for x in range(sw):
            if fourcc in LUMA_FIRST:
                S[y, x] = r[x]
            elif fourcc in YUV422:
                S[y, x] = r[2 * x + YUV422[fourcc]]
            else:
                bpp, ri, gi, bi = RGB_ORDER[fourcc]
                S[y, x] = L(r[bpp * x + ri], r[bpp * x + gi], r[bpp * x + bi])
    return S


def luma_vec(buf, fourcc, sw, sh, stride):
    b = np.asarray(buf, np.uint8).reshape(-1)
    need = (sh - 1) * stride + min_stride(fourcc, sw)
    rows = np.lib.stride_tricks.as_strided(b[:need], (sh, min_stride(fourcc, sw)), (stride, 1))
    if fourcc in LUMA_FIRST:
        return rows[:, :sw].copy()
    if fourcc in YUV422:
        return rows[:, YUV422[fourcc]:2 * sw:2].copy()
    bpp, ri, gi, bi = RGB_ORDER[fourcc]
    px = rows[:, :bpp * sw].reshape(sh, sw, bpp)
    return L(px[:, :, ri], px[:, :, gi], px[:, :, bi])


def orient(S, o):
    """The oriented frame of the source luma S[sh][sw], the contract's four cases as loops."""
    o = ORIENT_CODE[o] if isinstance(o, str) else o
    sh, sw = S.shape
    W, H = (sh, sw) if o in (1, 3) else (sw, sh)
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if o == 0:
                out[y, x] = S[y, x]
            elif o == 1:
                out[y, x] = S[sh - 1 - x, y]
            elif o == 2:
                out[y, x] = S[sh - 1 - y, sw - 1 - x]
            else:
                out[y, x] = S[x, sw - 1 - y]
    return out


def orient_vec(S, o):
    o = ORIENT_CODE[o] if isinstance(o, str) else o
    return np.ascontiguousarray((S, np.rot90(S, -1), S[::-1, ::-1], np.rot90(S, 1))[o])


def expected(buf, fourcc, sw, sh, stride, o):
    """What the device must stage for one source frame."""
    return orient_vec(luma_vec(buf, fourcc, sw, sh, stride), o)


def source_of(frame, o):
    """The source luma S whose orientation by `o` is `frame` (the inverse turn): orient_vec(source_of(f, o), o) == f."""
    o = ORIENT_CODE[o] if isinstance(o, str) else o
    return np.ascontiguousarray((frame, np.rot90(frame, 1), frame[::-1, ::-1], np.rot90(frame, -1))[o])


def grey_to_rgb(frame, seed=0):
    """An RGB image whose luma is close to `frame` but not grey: the channels are spread around it."""
    rng = np.random.default_rng(seed)
    f = frame.astype(np.int32)
    d = rng.integers(-20, 21, frame.shape + (2,))
    r, b = np.clip(f + d[..., 0], 0, 255), np.clip(f + d[..., 1], 0, 255)
    g = np.clip((f * 65536 - 19595 * r - 7471 * b) // 38470, 0, 255)
    return np.stack([r, g, b], -1).astype(np.uint8)
