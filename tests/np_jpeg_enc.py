"""numpy restatement of the preview path (chalkydri_hip.h: ck_preview_jpeg): nearest-neighbour scale, the
detection overlay, and a 1-component baseline JPEG encoder that restates libjpeg — jpeg_fdct_islow, its quantiser, the Annex-K
luminance Huffman tables, restart intervals and Pillow's header for mode L — so that a file equals libjpeg(-turbo)'s byte for
byte.  Depends on numpy and tests/np_jpeg.py only: the GPU tests compare against it."""
import numpy as np

import np_jpeg as J

MJPEG_PREFIX = b"--frame\r\nContent-Length: "
MJPEG_MIDDLE = b"\r\nContent-Type: image/jpeg\r\n\r\n"
BLOCK_MAX_BYTES = 264   # a baseline block before stuffing: 68 symbols of at most 31 bits


# ---- geometry (ck_preview_layout) -------------------------------------------------------------------------------------------
def header_len(restart_rows):
    # SOI 2, APP0 18, DQT 69, SOF0 13, DHT DC 33, DHT AC 183, DRI 6 (only with a restart interval), SOS 10
    return 2 + 18 + 69 + 13 + 33 + 183 + (6 if restart_rows else 0) + 10


def layout(width, height, W, H, quality=50, restart_rows=0):
    """(pw, ph, max_bytes) or None where the library answers CK_EINVAL."""
    if W < 1 or H < 1 or width < 0 or height < 0 or not 1 <= quality <= 100 or restart_rows < 0:
        return None
    pw = W if width == 0 or width > W else width
    ph = H if height == 0 or height > H else height
    if pw < 8 or ph < 8:
        return None
    bw, bh = -(-pw // 8), -(-ph // 8)
    if restart_rows * bw > 65535:
        return None
    nint = -(-bh // restart_rows) if restart_rows else 1
    return pw, ph, header_len(restart_rows) + 2 * (bw * bh * BLOCK_MAX_BYTES + nint) + 2 * (nint - 1) + 2


# ---- scale ------------------------------------------------------------------------------------------------------------------
def scale_nn(F, pw, ph):
    """P[y][x] = F[(2y+1) H / (2 ph)][(2x+1) W / (2 pw)]: pixel-centre nearest neighbour in integers."""
    F = np.asarray(F, np.uint8)
    H, W = F.shape
    sy = ((2 * np.arange(ph, dtype=np.int64) + 1) * H) // (2 * ph)
    sx = ((2 * np.arange(pw, dtype=np.int64) + 1) * W) // (2 * pw)
    return np.ascontiguousarray(F[sy][:, sx])


# ---- overlay ----------------------------------------------------------------------------------------------------------------
def corner_pixel(p, pw, ph, W, H):
    """One multiplication, one division, floor, in double; then clamped to the preview."""
    ix = np.floor(np.float64(p[0]) * np.float64(pw) / np.float64(W))
    iy = np.floor(np.float64(p[1]) * np.float64(ph) / np.float64(H))
    return int(min(max(ix, 0.0), pw - 1.0)), int(min(max(iy, 0.0), ph - 1.0))


def line_pixels(a, b):
    """Integer Bresenham between two pixels, both included.  The line is always walked from the end point that is smaller in
    (y, x) order, so a -> b and b -> a give the same pixels; with dx = |x1 - x0|, dy = -|y1 - y0|, err = dx + dy each step
    doubles err and moves in x when 2 err >= dy, in y when 2 err <= dx (both on a diagonal step)."""
    (x0, y0), (x1, y1) = (a, b) if (a[1], a[0]) <= (b[1], b[0]) else (b, a)
    dx, dy = abs(x1 - x0), -abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err = dx + dy
    out = []
    while True:
        out.append((x0, y0))
        if x0 == x1 and y0 == y1:
            return out
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x0 += sx
        if e2 <= dx:
            err += dx
            y0 += sy


def overlay_mask(dets, pw, ph, W, H):
    """dets: corner arrays [4][2] in frame pixels (Detection.corners()).  bool [ph][pw]: every pixel of every outline."""
    m = np.zeros((ph, pw), bool)
    for p in dets:
        p = np.asarray(p, np.float64)
        c = [corner_pixel(p[k], pw, ph, W, H) for k in range(4)]
        for k in range(4):
            for x, y in line_pixels(c[k], c[(k + 1) & 3]):
                m[y, x] = True
    return m


def apply_overlay(P, mask):
    P = np.asarray(P, np.uint8)
    return np.where(mask, np.where(P < 128, 255, 0), P).astype(np.uint8)


def preview(F, pw, ph, dets=None):
    """The pixels the encoder is given: scale, then the overlay of `dets` (None = no overlay)."""
    P = scale_nn(F, pw, ph)
    if dets is None:
        return P
    H, W = np.asarray(F).shape
    return apply_overlay(P, overlay_mask(dets, pw, ph, W, H))


# ---- encoder ----------------------------------------------------------------------------------------------------------------
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """jpeg_fdct_islow's 1-D pass along the last axis on int64 (CONST_BITS 13, PASS1_BITS 2)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    tmp0, tmp7, tmp1, tmp6 = d0 + d7, d0 - d7, d1 + d6, d1 - d6
    tmp2, tmp5, tmp3, tmp4 = d2 + d5, d2 - d5, d3 + d4, d3 - d4
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = 11 if first else 15
    if first:
        o0, o4 = (tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2
    else:
        o0, o4 = _descale(tmp10 + tmp11, 2), _descale(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * 4433
    o2 = _descale(z1 + tmp13 * 6270, n)
    o6 = _descale(z1 + tmp12 * -15137, n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o7, o5 = _descale(tmp4 + z1 + z3, n), _descale(tmp5 + z2 + z4, n)
    o3, o1 = _descale(tmp6 + z2 + z3, n), _descale(tmp7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], axis=-1)


def fdct_islow(blocks):
    """[n][8][8] level-shifted samples -> [n][8][8] coefficients scaled by 8 (rows first, then columns), int64."""
    rows = _fdct_1d(np.asarray(blocks, np.int64), True)
    return _fdct_1d(rows.transpose(0, 2, 1), False).transpose(0, 2, 1)


def quantise(coef, q):
    """libjpeg's quantiser for the islow FDCT: divisor 8 q, sign-magnitude, (|c| + qval / 2) / qval.  [n][64] natural order."""
    qv = 8 * np.asarray(q, np.int64).reshape(1, 64)
    c = np.asarray(coef, np.int64).reshape(-1, 64)
    return np.sign(c) * ((np.abs(c) + (qv >> 1)) // qv)


def blocks_of(P):
    """[bh * bw][8][8] level-shifted blocks of P, right / bottom edge replicated to whole blocks; (blocks, bw, bh)."""
    P = np.asarray(P, np.uint8)
    h, w = P.shape
    bw, bh = -(-w // 8), -(-h // 8)
    Y = np.pad(P.astype(np.int64), ((0, bh * 8 - h), (0, bw * 8 - w)), mode="edge") - 128
    return Y.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8), bw, bh


def quantised_zigzag(P, quality):
    B, bw, bh = blocks_of(P)
    return quantise(fdct_islow(B), J.quant_table(quality))[:, J.ZIGZAG], bw, bh


def _nbits(a):
    a = np.abs(a)
    n = np.zeros(a.shape, np.int64)
    for k in range(12):
        n += (a >> k) > 0
    return n


def header(w, h, quality, restart_interval):
    """Pillow's (libjpeg's) header for mode L, optimize=False."""
    out = bytearray(b"\xff\xd8")

    def seg(m, body):
        out.extend(bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + bytes(body))
    seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    seg(0xDB, bytes([0]) + bytes(int(v) for v in J.quant_table(quality)[J.ZIGZAG]))
    seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([1, 1, 0x11, 0]))
    seg(0xC4, bytes([0x00]) + bytes(J.STD_DC_BITS[0]) + bytes(range(12)))
    seg(0xC4, bytes([0x10]) + bytes(J.STD_AC_BITS[0]) + J.STD_AC_VALS[0])
    if restart_interval:
        seg(0xDD, int(restart_interval).to_bytes(2, "big"))
    seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0]))
    return bytes(out)


def _table_arrays():
    dcc, acc = J._codes(*J.STD_TABLES[(0, 0)]), J._codes(*J.STD_TABLES[(1, 0)])
    dc = np.zeros((16, 2), np.int64)
    ac = np.zeros((256, 2), np.int64)
    for sym, cl in dcc.items():
        dc[sym] = cl
    for sym, cl in acc.items():
        ac[sym] = cl
    return dc, ac


_DC, _AC = _table_arrays()


def _pack(values, lengths):
    """MSB-first concatenation of (value, length <= 16) items, the last byte padded with 1-bits (np_jpeg.pack_bits' result,
    assembled in 32-bit words so that a whole frame is one call)."""
    l = np.asarray(lengths, np.int64)
    keep = l > 0
    v, l = np.asarray(values, np.int64)[keep], l[keep]
    total = int(l.sum())
    if total == 0:
        return b""
    pad = (-total) % 8
    if pad:
        v, l = np.append(v, (1 << pad) - 1), np.append(l, pad)
    off = np.cumsum(l) - l
    w = off >> 5
    x = v << (64 - (off & 31) - l)                      # the item inside a 64-bit window that starts at word w
    nw = (total + pad + 31) // 32 + 1
    # the items' bits are disjoint, so sums are ORs; every sum is below 2^32 and exact in float64
    words = np.bincount(w, (x >> 32).astype(np.float64), nw) + np.bincount(w + 1, (x & 0xFFFFFFFF).astype(np.float64), nw)
    return words.astype(np.uint32).astype(">u4").tobytes()[:(total + pad) // 8]


def entropy_items(Z, R):
    """(values, lengths) [nblk][318] of the blocks' Huffman items in stream order: DC code, DC bits, then per zig-zag position
    1..63 three ZRL slots, the (run, size) code and the value bits, then EOB; unused slots have length 0.  R: blocks per
    restart interval (the DC prediction restarts with it)."""
    Z = np.asarray(Z, np.int64)
    nblk = Z.shape[0]
    V = np.zeros((nblk, 318), np.int64)
    L = np.zeros((nblk, 318), np.int64)
    prev = np.concatenate([[0], Z[:-1, 0]])
    prev[np.arange(nblk) % R == 0] = 0
    diff = Z[:, 0] - prev
    s = _nbits(diff)
    V[:, 0], L[:, 0] = _DC[s, 0], _DC[s, 1]
    V[:, 1], L[:, 1] = np.where(diff > 0, diff, diff + (1 << s) - 1), s
    idx = np.arange(64, dtype=np.int64)[None, :]
    nz = Z != 0
    nz[:, 0] = True                                        # runs are counted from the DC's position
    last = np.maximum.accumulate(np.where(nz, idx, 0), axis=1)
    run = (idx - 1 - np.concatenate([np.zeros((nblk, 1), np.int64), last[:, :-1]], axis=1))[:, 1:]
    ac = Z[:, 1:]
    on = ac != 0
    s = _nbits(ac)
    zrl = np.where(on, run >> 4, 0)
    for k in range(3):
        V[:, 2 + k:317:5] = np.where(zrl > k, _AC[0xF0, 0], 0)
        L[:, 2 + k:317:5] = np.where(zrl > k, _AC[0xF0, 1], 0)
    sym = np.where(on, ((run & 15) << 4) | s, 0)
    V[:, 5:317:5] = np.where(on, _AC[sym, 0], 0)
    L[:, 5:317:5] = np.where(on, _AC[sym, 1], 0)
    V[:, 6:317:5] = np.where(on, np.where(ac > 0, ac, ac + (1 << s) - 1), 0)
    L[:, 6:317:5] = np.where(on, s, 0)
    eob = last[:, 63] < 63
    V[:, 317], L[:, 317] = np.where(eob, _AC[0, 0], 0), np.where(eob, _AC[0, 1], 0)
    return V, L


def encode_grey(P, quality=50, restart_rows=0):
    """The complete file libjpeg writes for the 8-bit image P [h][w]: quality via jpeg_set_quality (baseline), no optimised
    tables, restart interval = restart_rows block rows (0 = none)."""
    P = np.asarray(P, np.uint8)
    h, w = P.shape
    Z, bw, bh = quantised_zigzag(P, quality)
    nblk = bw * bh
    R = restart_rows * bw if restart_rows else nblk
    V, L = entropy_items(Z, R)
    scan = bytearray()
    for k in range(-(-nblk // R)):
        if k:
            scan += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        scan += J.stuff(_pack(V[k * R:(k + 1) * R].reshape(-1), L[k * R:(k + 1) * R].reshape(-1)))
    return header(w, h, quality, restart_rows * bw if restart_rows else 0) + bytes(scan) + b"\xff\xd9"


def mjpeg_part(jpeg):
    """One part of the driver-station stream: the multipart framing in front of a complete JPEG."""
    jpeg = bytes(jpeg)
    return MJPEG_PREFIX + str(len(jpeg)).encode("ascii") + MJPEG_MIDDLE + jpeg
