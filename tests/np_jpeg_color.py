"""numpy restatement of the colour form of the JPEG decode (chalkydri_hip.h: ck_upload_jpeg_color): the frame C of
(Y, Cb, Cr) triples of a stream — Y as np_jpeg.decode_luma gives it, Cb and Cr from the component's own plane (jpeg_idct_islow
with its own quantisation table, the masked range limit) through libjpeg's fancy upsampling in integers; Cb = Cr = 128 for a
one-component stream; (0, 128, 128) for a frame that fails.  Then the preview's end-to-end reference: orient, scale, overlay
(raw_format_ref, preview_color_ref's steps) and Pillow's encoding of the YCbCr picture.  np_jpeg's parse, tables and idct_islow
are used as they are."""
import io

import numpy as np

import np_jpeg as J
import np_jpeg_enc as E
import np_jpeg_enc_color as EC
import raw_format_ref as R


def component_tables(data):
    """[quantisation table (natural order)] per component of the frame, by the Tq of its SOF entry (np_jpeg.parse keeps Y's only).
    The stream has passed np_jpeg.parse, so every segment is well formed."""
    d = bytes(data)
    i, qt, tq = 2, {}, []
    while True:
        while d[i] != 0xFF:
            i += 1
        while d[i] == 0xFF:
            i += 1
        m = d[i]
        i += 1
        if m in (0, 1) or 0xD0 <= m <= 0xD7:
            continue
        L = (d[i] << 8) | d[i + 1]
        s = d[i + 2:i + L]
        i += L
        if m == 0xDB:
            o = 0
            while o < len(s):
                pq, t = s[o] >> 4, s[o] & 15
                q = np.zeros(64, np.int64)
                for k in range(64):
                    q[J.ZIGZAG[k]] = (s[o + 1 + 2 * k] << 8 | s[o + 2 + 2 * k]) if pq else s[o + 1 + k]
                qt[t] = q
                o += 1 + 64 * (pq + 1)
        elif m in (0xC0, 0xC1):
            tq = [s[8 + 3 * c] for c in range(s[5])]
        elif m == 0xDA:
            return [qt[t] for t in tq]


def decode_planes(data):
    """(Y [h][w], Cb plane [ch][cw] or None, Cr plane or None, (hs, vs), status): np_jpeg.decode_luma's walk over the scan with the
    chroma blocks kept — one block per MCU and component, raster order over the MCUs, DC prediction per component restarting with
    every interval — and their planes cropped to cw x ch = ceil(w / hs) x ceil(h / vs).  A frame that fails: (zeros, None, None)."""
    try:
        P = J.parse(data)
    except J.JpegError as e:
        return np.zeros((0, 0), np.uint8), None, None, (1, 1), (J.UNSUPPORTED if e.code == "EUNSUPPORTED" else J.CORRUPT)
    w, h, nc = P["width"], P["height"], P["n_components"]
    H, V = (P["h_samp"], P["v_samp"]) if nc == 3 else (1, 1)
    nyb = H * V
    bpm = nyb + 2 if nc == 3 else 1
    mcux, mcuy = -(-w // (8 * H)), -(-h // (8 * V))
    nmcu = mcux * mcuy
    Rst = P["restart_interval"] or nmcu
    nint = -(-nmcu // Rst)
    fail = (np.zeros((h, w), np.uint8), None, None, (H, V), J.CORRUPT)
    comp, rst = J.unstuff(bytes(data)[P["scan_off"]:])
    if len(rst) != nint - 1 or any(r != (k & 7) for k, (_, r) in enumerate(rst)):
        return fail
    starts = [0] + [o for o, _ in rst] + [len(comp)]
    c = np.frombuffer(comp + b"\xff" * 8, np.uint8).astype(np.int64)
    win = ((c[:-3] << 24) | (c[1:-2] << 16) | (c[2:-1] << 8) | c[3:]).tolist()
    far = len(comp) * 8 + 32

    def peek(p, nbits):   # bits past the scan read as ones
        if p >= far:
            return (1 << nbits) - 1
        return ((win[p >> 3] << (p & 7)) & 0xFFFFFFFF) >> (32 - nbits)
    luts = [(J._lut16(*dct), J._lut16(*act)) for dct, act in P["tables"]]
    nat = J.ZIGZAG.tolist()
    ystride = mcux * H
    coef = [[[0] * 64 for _ in range(nmcu * nyb)], [[0] * 64 for _ in range(nmcu)], [[0] * 64 for _ in range(nmcu)]]
    for k in range(nint):
        pos, lim = starts[k] * 8, starts[k + 1] * 8
        last = [0, 0, 0]
        for b in range(min(Rst, nmcu - k * Rst) * bpm):
            mcu, sl = k * Rst + b // bpm, b % bpm
            ci = 0 if sl < nyb else sl - nyb + 1
            dcl, acl = luts[ci]
            if ci == 0:
                my, mx = divmod(mcu, mcux)
                blk = coef[0][(my * V + sl // H) * ystride + mx * H + sl % H]
            else:
                blk = coef[ci][mcu]
            e = dcl[peek(pos, 16)]
            if not e:
                return fail
            pos += e >> 8
            s = e & 255
            if s:
                v = peek(pos, s)
                pos += s
                last[ci] += v if v >= (1 << (s - 1)) else v - (1 << s) + 1
            blk[0] = last[ci]
            kk = 1
            while kk < 64:
                e = acl[peek(pos, 16)]
                if not e:
                    return fail
                pos += e >> 8
                r, s = (e & 255) >> 4, e & 15
                if s:
                    kk += r
                    if kk > 63:
                        return fail
                    v = peek(pos, s)
                    pos += s
                    blk[nat[kk]] = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                    kk += 1
                elif r == 15:
                    if kk + 15 > 63:
                        return fail
                    kk += 16
                else:
                    break
            if pos > lim:     # the interval ends before its MCUs do
                return fail
    qts = component_tables(data)

    def plane(cf, q, brows, bcols, ph, pw):
        a = np.array(cf, np.int64)
        a = (a + 32768) % 65536 - 32768                             # libjpeg stores coefficients as 16-bit JCOEFs
        pix = J.idct_islow(a, q).reshape(brows, bcols, 8, 8).transpose(0, 2, 1, 3).reshape(brows * 8, bcols * 8)
        return np.ascontiguousarray(pix[:ph, :pw])
    Y = plane(coef[0], qts[0], mcuy * V, mcux * H, h, w)
    if nc == 1:
        return Y, None, None, (1, 1), J.OK
    cw, ch = -(-w // H), -(-h // V)
    return Y, plane(coef[1], qts[1], mcuy, mcux, ch, cw), plane(coef[2], qts[2], mcuy, mcux, ch, cw), (H, V), J.OK


def upsample(P, hs, vs, w, h):
    """The contract's four formulas as loops: component value at every pixel (x, y) of the w x h frame from the plane P [ch][cw]."""
    P = np.asarray(P, np.int64)
    ch, cw = P.shape
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        j = y >> 1
        jn = max(j - 1, 0) if y % 2 == 0 else min(j + 1, ch - 1)
        for x in range(w):
            i = x >> 1
            if (hs, vs) == (1, 1):
                v = P[y][x]
            elif (hs, vs) == (2, 1):
                if x % 2 == 0:
                    v = P[y][0] if x == 0 else (3 * P[y][i] + P[y][i - 1] + 1) >> 2
                else:
                    v = P[y][cw - 1] if x == 2 * cw - 1 else (3 * P[y][i] + P[y][i + 1] + 2) >> 2
            elif (hs, vs) == (1, 2):
                v = (3 * P[j][x] + P[jn][x] + (1 if y % 2 == 0 else 2)) >> 2
            else:
                T = lambda k: 3 * P[j][k] + P[jn][k]  # noqa: E731
                if x % 2 == 0:
                    v = (4 * T(0) + 8) >> 4 if x == 0 else (3 * T(i) + T(i - 1) + 8) >> 4
                else:
                    v = (4 * T(cw - 1) + 7) >> 4 if x == 2 * cw - 1 else (3 * T(i) + T(i + 1) + 7) >> 4
            out[y, x] = v
    return out


def upsample_vec(P, hs, vs, w, h):
    """upsample, vectorised (the host test ties it to the loops)."""
    P = np.asarray(P, np.int64)
    ch, cw = P.shape
    y, x = np.arange(h), np.arange(w)
    if vs == 2:
        j = y >> 1
        jn = np.where(y % 2 == 0, np.maximum(j - 1, 0), np.minimum(j + 1, ch - 1))
        T = 3 * P[j] + P[jn]                                         # [h][cw]
        if hs == 1:
            return ((T + np.where(y % 2 == 0, 1, 2)[:, None]) >> 2).astype(np.uint8)[:, :w]
    else:
        T = P[:h]
        if hs == 1:
            return T[:, :w].astype(np.uint8)
    i = x >> 1
    inn = np.where(x % 2 == 0, np.maximum(i - 1, 0), np.minimum(i + 1, cw - 1))   # at the two ends the neighbour is the sample itself
    if vs == 1:
        return ((3 * T[:, i] + T[:, inn] + np.where(x % 2 == 0, 1, 2)[None, :]) >> 2).astype(np.uint8)
    return ((3 * T[:, i] + T[:, inn] + np.where(x % 2 == 0, 8, 7)[None, :]) >> 4).astype(np.uint8)


def decode_color(data, size=None, up=upsample_vec):
    """(C [sh][sw][3] uint8, status) under the library's rules.  size = (sw, sh): the handle's source geometry; a stream of another
    size is CK_JPEG_GEOMETRY.  A frame that fails is (0, 128, 128) everywhere ([0][0][3] when no size is known)."""
    Y, Cb, Cr, (hs, vs), st = decode_planes(data)
    if st == J.OK and size is not None and (Y.shape[1], Y.shape[0]) != tuple(size):
        st = J.GEOMETRY
    if size is not None and st != J.OK:
        Y = np.zeros((size[1], size[0]), np.uint8)
    h, w = Y.shape
    C = np.full((h, w, 3), 128, np.uint8)
    C[..., 0] = Y if st == J.OK else 0
    if st == J.OK and Cb is not None:
        C[..., 1] = up(Cb, hs, vs, w, h)
        C[..., 2] = up(Cr, hs, vs, w, h)
    return C, st


def preview_triples(C, o, pw, ph, dets=None):
    """P [ph][pw][3]: orient(C) by §4d's index maps, the nearest-neighbour scale and the overlay of §4g."""
    O = R.orient_vec(C, o)
    H, W = O.shape[:2]
    sy = ((2 * np.arange(ph, dtype=np.int64) + 1) * H) // (2 * ph)
    sx = ((2 * np.arange(pw, dtype=np.int64) + 1) * W) // (2 * pw)
    P = np.ascontiguousarray(O[sy][:, sx])
    if dets is not None:
        P[E.overlay_mask(dets, pw, ph, W, H)] = EC.OVERLAY_TRIPLE
    return P


def pillow_file(P, quality=50, restart_rows=0):
    """The file libjpeg writes for the YCbCr picture P: 4:4:4, baseline, the standard tables, no optimisation."""
    from PIL import Image
    buf = io.BytesIO()
    kw = {"restart_marker_rows": restart_rows} if restart_rows else {}
    Image.fromarray(np.ascontiguousarray(P), "YCbCr").save(buf, "JPEG", quality=quality, subsampling=0, **kw)
    return buf.getvalue()


def pillow_ycc(data):
    """Pillow's (libjpeg-turbo's) decode of a stream to YCbCr without colour conversion: the oracle of decode_color."""
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(data)))
    if im.mode == "L":
        Y = np.asarray(im)
        return np.stack([Y, np.full_like(Y, 128), np.full_like(Y, 128)], -1)
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr", im.mode
    return np.asarray(im)
