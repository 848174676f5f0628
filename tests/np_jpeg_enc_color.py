"""numpy restatement of the colour preview's encoder (chalkydri_hip.h: ck_preview_jpeg_color): a
three-component 4:4:4 interleaved baseline JPEG as libjpeg writes it from YCbCr input — MCU = Y block, Cb block, Cr block;
jpeg_fdct_islow and the quantiser of tests/np_jpeg_enc.py with table 0 for Y and the chrominance table for Cb and Cr; DC
prediction per component, restarting with every interval; the Annex-K luminance Huffman tables for Y, the chrominance tables for
Cb and Cr; Pillow's header for modes RGB and YCbCr.  Also libjpeg's rgb_ycc_convert.  Depends on numpy, tests/np_jpeg.py and
tests/np_jpeg_enc.py only: the GPU tests compare against it, tests/test_preview_color_host.py ties it to Pillow."""
import numpy as np

import np_jpeg as J
import np_jpeg_enc as E


# ---- libjpeg's rgb_ycc_convert (jccolor.c), 16-bit fixed point in signed 32-bit arithmetic ----------------------------------------
def ycc(r, g, b):
    """(Y, Cb, Cr) uint8 of R, G, B uint8 (arrays or scalars)."""
    r, g, b = (np.asarray(v).astype(np.int32) for v in (r, g, b))
    half = (128 << 16) + 32767
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + half) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + half) >> 16
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def rgb_to_ycc(rgb):
    """[h][w][3] RGB -> [h][w][3] (Y, Cb, Cr)."""
    rgb = np.asarray(rgb, np.uint8)
    return np.stack(ycc(rgb[..., 0], rgb[..., 1], rgb[..., 2]), -1)


OVERLAY_TRIPLE = tuple(int(v) for v in ycc(0, 255, 0))   # RGB (0, 255, 0): (150, 44, 21)


# ---- geometry (ck_preview_color_layout) -------------------------------------------------------------------------------------------
def header_len(restart_rows):
    # SOI 2, APP0 18, DQT 69 x 2, SOF0 19, (DHT DC 33, DHT AC 183) x 2, DRI 6 (only with a restart interval), SOS 14
    return 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + (6 if restart_rows else 0) + 14


def layout(width, height, W, H, quality=50, restart_rows=0):
    """(pw, ph, max_bytes) or None where the library answers CK_EINVAL: the grey layout with three times the blocks."""
    grey = E.layout(width, height, W, H, quality, restart_rows)
    if grey is None:
        return None
    pw, ph, _ = grey
    bw, bh = -(-pw // 8), -(-ph // 8)
    nint = -(-bh // restart_rows) if restart_rows else 1
    return pw, ph, header_len(restart_rows) + 2 * (3 * bw * bh * E.BLOCK_MAX_BYTES + nint) + 2 * (nint - 1) + 2


# ---- encoder ----------------------------------------------------------------------------------------------------------------------
def header(w, h, quality, restart_interval):
    """Pillow's (libjpeg's) header for modes RGB and YCbCr, optimize=False, subsampling 4:4:4."""
    out = bytearray(b"\xff\xd8")

    def seg(m, body):
        out.extend(bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + bytes(body))
    seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2):
        seg(0xDB, bytes([t]) + bytes(int(v) for v in J.quant_table(quality, t)[J.ZIGZAG]))
    seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for t in range(2):
        seg(0xC4, bytes([0x00 | t]) + bytes(J.STD_DC_BITS[t]) + bytes(range(12)))
        seg(0xC4, bytes([0x10 | t]) + bytes(J.STD_AC_BITS[t]) + J.STD_AC_VALS[t])
    if restart_interval:
        seg(0xDD, int(restart_interval).to_bytes(2, "big"))
    seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return bytes(out)


def _table_arrays(t):
    dc = np.zeros((16, 2), np.int64)
    ac = np.zeros((256, 2), np.int64)
    for sym, cl in J._codes(*J.STD_TABLES[(0, t)]).items():
        dc[sym] = cl
    for sym, cl in J._codes(*J.STD_TABLES[(1, t)]).items():
        ac[sym] = cl
    return dc, ac


TABLES = [_table_arrays(0), _table_arrays(1)]   # [luminance, chrominance] x (DC, AC): [symbol] = (code, length)
ITEMS = 2 + 63 * 5 + 1                           # slots per block: DC code, DC bits, 63 x (3 ZRL, code, bits), EOB


def worst_block_bits(t):
    """An upper bound of a block's bits under table set t: the longest DC item, 63 times the longest (code + value bits) of an AC
    symbol (a block of 63 coefficients has no room for ZRL or EOB; one with fewer trades at least one such item for a ZRL, which
    is shorter)."""
    dc, ac = TABLES[t]
    longest_dc = max(int(dc[s, 1]) + s for s in range(12))
    longest_ac = max(int(ac[(r << 4) | s, 1]) + s for r in range(16) for s in range(1, 11))
    assert int(ac[0xF0, 1]) <= longest_ac and int(ac[0, 1]) <= longest_ac
    return longest_dc + 63 * longest_ac


def entropy_items(Z, R, t):
    """(values, lengths) [nblk][ITEMS] of the Huffman items of ONE component's blocks Z [nblk][64] (zig-zag order) in stream
    order, under table set t; the DC prediction runs along the component's blocks and restarts every R of them."""
    dc, ac = TABLES[t]
    Z = np.asarray(Z, np.int64)
    nblk = Z.shape[0]
    V = np.zeros((nblk, ITEMS), np.int64)
    L = np.zeros((nblk, ITEMS), np.int64)
    prev = np.concatenate([[0], Z[:-1, 0]])
    prev[np.arange(nblk) % R == 0] = 0
    diff = Z[:, 0] - prev
    s = E._nbits(diff)
    V[:, 0], L[:, 0] = dc[s, 0], dc[s, 1]
    V[:, 1], L[:, 1] = np.where(diff > 0, diff, diff + (1 << s) - 1), s
    for b in range(nblk):                      # plain loops over the AC positions: the run-length rule as T.81 F.1.2.2 states it
        run, k = 0, 2
        for pos in range(1, 64):
            v = int(Z[b, pos])
            if v == 0:
                run += 1
                k += 5
                continue
            for z in range(run >> 4):
                V[b, k + z], L[b, k + z] = ac[0xF0]
            size = abs(v).bit_length()
            V[b, k + 3], L[b, k + 3] = ac[((run & 15) << 4) | size]
            V[b, k + 4], L[b, k + 4] = (v if v > 0 else v + (1 << size) - 1), size
            run = 0
            k += 5
        if run:
            V[b, ITEMS - 1], L[b, ITEMS - 1] = ac[0]
    return V, L


def entropy_items_vec(Z, R, t):
    """entropy_items without the loops over blocks (np_jpeg_enc.entropy_items' arithmetic with the tables of set t)."""
    dc, ac = TABLES[t]
    Z = np.asarray(Z, np.int64)
    nblk = Z.shape[0]
    V = np.zeros((nblk, ITEMS), np.int64)
    L = np.zeros((nblk, ITEMS), np.int64)
    prev = np.concatenate([[0], Z[:-1, 0]])
    prev[np.arange(nblk) % R == 0] = 0
    diff = Z[:, 0] - prev
    s = E._nbits(diff)
    V[:, 0], L[:, 0] = dc[s, 0], dc[s, 1]
    V[:, 1], L[:, 1] = np.where(diff > 0, diff, diff + (1 << s) - 1), s
    idx = np.arange(64, dtype=np.int64)[None, :]
    nz = Z != 0
    nz[:, 0] = True
    last = np.maximum.accumulate(np.where(nz, idx, 0), axis=1)
    run = (idx - 1 - np.concatenate([np.zeros((nblk, 1), np.int64), last[:, :-1]], axis=1))[:, 1:]
    a = Z[:, 1:]
    on = a != 0
    s = E._nbits(a)
    zrl = np.where(on, run >> 4, 0)
    for k in range(3):
        V[:, 2 + k:ITEMS - 1:5] = np.where(zrl > k, ac[0xF0, 0], 0)
        L[:, 2 + k:ITEMS - 1:5] = np.where(zrl > k, ac[0xF0, 1], 0)
    sym = np.where(on, ((run & 15) << 4) | s, 0)
    V[:, 5:ITEMS - 1:5] = np.where(on, ac[sym, 0], 0)
    L[:, 5:ITEMS - 1:5] = np.where(on, ac[sym, 1], 0)
    V[:, 6:ITEMS - 1:5] = np.where(on, np.where(a > 0, a, a + (1 << s) - 1), 0)
    L[:, 6:ITEMS - 1:5] = np.where(on, s, 0)
    eob = last[:, 63] < 63
    V[:, ITEMS - 1], L[:, ITEMS - 1] = np.where(eob, ac[0, 0], 0), np.where(eob, ac[0, 1], 0)
    return V, L


def encode_ycc(P, quality=50, restart_rows=0, items=entropy_items_vec):
    """The complete file libjpeg writes for the (Y, Cb, Cr) image P [h][w][3], 4:4:4: quality via jpeg_set_quality (baseline), no
    optimised tables, restart interval = restart_rows MCU rows (0 = none)."""
    P = np.asarray(P, np.uint8)
    h, w, _ = P.shape
    bw, bh = -(-w // 8), -(-h // 8)
    nmcu = bw * bh
    R = restart_rows * bw if restart_rows else nmcu                      # MCUs per interval
    V = np.zeros((nmcu, 3, ITEMS), np.int64)
    L = np.zeros((nmcu, 3, ITEMS), np.int64)
    for c in range(3):
        B, _, _ = E.blocks_of(P[:, :, c])
        Z = E.quantise(E.fdct_islow(B), J.quant_table(quality, 1 if c else 0))[:, J.ZIGZAG]
        V[:, c], L[:, c] = items(Z, R, 1 if c else 0)
    scan = bytearray()
    for k in range(-(-nmcu // R)):
        if k:
            scan += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        scan += J.stuff(E._pack(V[k * R:(k + 1) * R].reshape(-1), L[k * R:(k + 1) * R].reshape(-1)))
    return header(w, h, quality, restart_rows * bw if restart_rows else 0) + bytes(scan) + b"\xff\xd9"
