"""numpy baseline JPEG: an encoder that writes every layout the device decoder supports, and a luma-only decoder that restates
libjpeg's Huffman decode and integer ("islow") IDCT exactly, with the library's per-frame failure rules (chalkydri_hip.h:
ck_upload_jpeg).  Depends on numpy only: the GPU tests compare against it."""
import numpy as np

OK, UNSUPPORTED, GEOMETRY, CORRUPT = 0, 1, 2, 4

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63])   # zig-zag index -> natural index

# ITU-T T.81 Annex K: quantisation (K.1) and Huffman (K.3) tables.  bits[l] = codes of length l + 1.
STD_Q = (np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
                   51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                   101, 72, 92, 95, 98, 112, 100, 103, 99]),
         np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                   99, 99, 99, 99] + [99] * 32))
STD_DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
STD_AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
STD_AC_VALS = (
    bytes.fromhex("01020300041105122131410613516107227114328191a1082342b1c11552d1f0243362728209"
                  "0a161718191a25262728292a3435363738393a434445464748494a535455565758595a636465"
                  "666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
                  "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9ea"
                  "f1f2f3f4f5f6f7f8f9fa"),
    bytes.fromhex("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a"
                  "162434e125f11718191a262728292a35363738393a434445464748494a535455565758595a"
                  "636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4"
                  "a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5"
                  "e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
STD_TABLES = {(0, 0): (STD_DC_BITS[0], list(range(12))), (0, 1): (STD_DC_BITS[1], list(range(12))),
              (1, 0): (STD_AC_BITS[0], list(STD_AC_VALS[0])), (1, 1): (STD_AC_BITS[1], list(STD_AC_VALS[1]))}
SAMPLINGS = {"444": (1, 1), "422": (2, 1), "440": (1, 2), "420": (2, 2), "grey": None}


class JpegError(Exception):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code   # "EINVAL" or "EUNSUPPORTED"


# ---- encoder ----------------------------------------------------------------------------------------------------------------
def quant_table(quality, which=0):
    """libjpeg's jpeg_set_quality scaling of the K.1 table (force_baseline: 1..255), natural order."""
    q = max(1, min(100, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((STD_Q[which] * scale + 50) // 100, 1, 255).astype(np.int64)


def _dct_matrix():
    k = np.arange(8)
    c = np.sqrt(2 / 8) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
    c[0] /= np.sqrt(2)
    return c


_C8 = _dct_matrix()


def _category(v):
    return int(abs(int(v))).bit_length()


def _codes(bits, vals):
    """canonical codes: {symbol: (code, length)}"""
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[p]] = (code, l)
            code += 1
            p += 1
        code <<= 1
    return out


def shuffled_table(cls, slot, rng):
    """A caller-given table: the standard code lengths with the symbols shuffled among them (valid and different)."""
    bits, vals = STD_TABLES[(cls, slot)]
    vals = list(vals)
    rng.shuffle(vals)
    return list(bits), vals


def pack_bits(values, lengths):
    """MSB-first concatenation of (value, length) items, padded with 1-bits to a whole byte."""
    v = np.asarray(values, np.int64)
    l = np.asarray(lengths, np.int64)
    total = int(l.sum())
    if total == 0:
        return b""
    start = np.repeat(np.cumsum(l) - l, l)
    shift = np.repeat(l, l) - 1 - (np.arange(total) - start)
    bits = (np.repeat(v, l) >> shift) & 1
    bits = np.concatenate([bits, np.ones((-total) % 8, np.int64)])
    return np.packbits(bits.astype(np.uint8)).tobytes()


def stuff(b):
    return bytes(b).replace(b"\xff", b"\xff\x00")


def encode(luma, sampling="420", quality=85, restart_interval=0, chroma=None, tables=None, dht=True, q16=False, restart_rows=False,
           dc_offset=0, append=None, fill=None, eob=0x00):
    """Baseline JPEG of an 8-bit luma plane [h][w] (+ chroma planes [h][w] each, derived from the luma when None).
    sampling: "444", "422", "440", "420" (Y sampling 1x1, 2x1, 1x2, 2x2) or "grey".  restart_interval in MCUs (restart_rows: in
    MCU rows).  tables: {(class, slot): (bits[16], vals)} replacing the K.3 tables; dht=False leaves every DHT out (the stream
    then relies on the standard tables); q16: write the quantisation tables with 16-bit precision.  dc_offset (a number, or numbers cycled over the
    blocks in raster order) is added to the quantised Y DCs (far out of the sample range with a coarse table: what reaches libjpeg's masked range limit).
    append: {interval index (negative: from the end): raw bytes written as they are after the interval's last code and its padding, before
    the marker that ends it}; fill: {interval index: number of 0xFF fill bytes in front of that marker}; eob: the symbol written where
    EOB stands in a component whose AC table holds it (an EOB-run symbol 0x10 .. 0xE0 of a caller-given table; 0x00 otherwise)."""
    luma = np.asarray(luma, np.uint8)
    h, w = luma.shape
    grey = sampling == "grey"
    H, V = (1, 1) if grey else SAMPLINGS[sampling]
    mcux, mcuy = -(-w // (8 * H)), -(-h // (8 * V))
    if restart_rows:
        restart_interval = mcux * restart_interval
    qt = [quant_table(quality, 0), quant_table(quality, 1)]
    T = dict(STD_TABLES)
    if tables:
        T.update(tables)
    # planes padded by edge replication to whole MCUs; chroma averaged over the sampling box
    Y = np.pad(luma.astype(np.int64), ((0, mcuy * 8 * V - h), (0, mcux * 8 * H - w)), mode="edge")
    comps = [(Y, H, V, 0)]
    if not grey:
        if chroma is None:
            chroma = (255 - luma, np.roll(luma, 3, axis=1))
        for pl in chroma:
            P = np.pad(np.asarray(pl, np.int64), ((0, mcuy * 8 * V - h), (0, mcux * 8 * H - w)), mode="edge")
            P = np.floor(P.reshape(mcuy * 8, V, mcux * 8, H).mean(axis=(1, 3)) + 0.5).astype(np.int64)
            comps.append((P, 1, 1, 1))
    # quantised coefficients per component in zig-zag order, [block row][block column][64]
    qcoef = []
    for P, ch, cv, t in comps:
        bh, bw = P.shape[0] // 8, P.shape[1] // 8
        B = (P - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8).astype(np.float64)
        D = _C8 @ B @ _C8.T
        Q = np.round(D.reshape(-1, 64) / qt[t][None, :]).astype(np.int64)
        if np.any(dc_offset) and len(qcoef) == 0:
            Q[:, 0] = np.clip(Q[:, 0] + np.resize(np.asarray(dc_offset, np.int64), Q.shape[0]), -2047, 2047)
        qcoef.append((Q[:, ZIGZAG].reshape(bh, bw, 64).tolist(), ch, cv, t))
    codes = {k: _codes(*v) for k, v in T.items()}
    nmcu = mcux * mcuy
    R = restart_interval or nmcu
    intervals, iv, il = [], [], []
    last = [0, 0, 0]
    for m in range(nmcu):
        if m % R == 0:
            if m:
                intervals.append((iv, il))
                iv, il = [], []
            last = [0, 0, 0]
        my, mx = divmod(m, mcux)
        for ci, (Q, ch, cv, t) in enumerate(qcoef):
            dcc, acc = codes[(0, t)], codes[(1, t)]
            for v in range(cv):
                for u in range(ch):
                    z = Q[my * cv + v][mx * ch + u]
                    dc = z[0] - last[ci]
                    last[ci] = z[0]
                    s = _category(dc)
                    c, l = dcc[s]
                    iv.append(c); il.append(l)
                    if s:
                        iv.append(dc if dc > 0 else dc + (1 << s) - 1); il.append(s)
                    k = 1
                    for idx in range(1, 64):
                        val = z[idx]
                        if not val:
                            continue
                        run = idx - k
                        while run > 15:
                            c, l = acc[0xF0]
                            iv.append(c); il.append(l)
                            run -= 16
                        s = _category(val)
                        c, l = acc[(run << 4) | s]
                        iv.append(c); il.append(l)
                        iv.append(val if val > 0 else val + (1 << s) - 1); il.append(s)
                        k = idx + 1
                    if k < 64:
                        c, l = acc[eob if eob in acc else 0x00]
                        iv.append(c); il.append(l)
    intervals.append((iv, il))
    scan = bytearray()
    for i, (vv, ll) in enumerate(intervals):
        if i:
            scan += bytes([0xFF, 0xD0 + ((i - 1) & 7)])
        scan += stuff(pack_bits(vv, ll))
        for extra, make in ((append, bytes), (fill, lambda n: b"\xff" * n)):
            for key in (i, i - len(intervals)):
                if extra and key in extra:
                    scan += make(extra[key])
    out = bytearray(b"\xff\xd8")

    def seg(m, body):
        out.extend(bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + bytes(body))
    for t in range(1 if grey else 2):
        body = bytearray([(0x10 if q16 else 0) | t])
        for k in range(64):
            body += int(qt[t][ZIGZAG[k]]).to_bytes(2 if q16 else 1, "big")
        seg(0xDB, body)
    sof = bytearray([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(comps)])
    for ci, (_, ch, cv, t) in enumerate(comps):
        sof += bytes([ci + 1, (ch << 4) | cv, t])
    seg(0xC0, sof)
    if dht:
        for (cls, slot) in sorted(T):
            if slot and grey:
                continue
            bits, vals = T[(cls, slot)]
            seg(0xC4, bytes([(cls << 4) | slot]) + bytes(bits) + bytes(vals))
    if restart_interval:
        seg(0xDD, int(restart_interval).to_bytes(2, "big"))
    sos = bytearray([len(comps)])
    for ci, (_, _, _, t) in enumerate(comps):
        sos += bytes([ci + 1, (t << 4) | t])
    seg(0xDA, sos + bytes([0, 63, 0]))
    out += scan + b"\xff\xd9"
    return bytes(out)


def strip_dht(data):
    """The stream without its DHT segments (what a UVC / AVI1 MJPEG frame looks like)."""
    d = bytes(data)
    out, i = bytearray(d[:2]), 2
    while i + 4 <= len(d) and d[i] == 0xFF:
        m, L = d[i + 1], (d[i + 2] << 8) | d[i + 3]
        if m != 0xC4:
            out += d[i:i + 2 + L]
        if m == 0xDA:
            return bytes(out) + d[i + 2 + L:]
        i += 2 + L
    return d


# ---- parser (the library's rules: chalkydri_hip.h ck_jpeg_info) -----------------------------------------------------------------
def parse(data):
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise JpegError("EINVAL", "not a JPEG")
    i, sof, restart, has_dht = 2, None, 0, False
    qt, dc, ac = {}, {}, {}
    while True:
        while i < n and d[i] != 0xFF:
            i += 1
        while i < n and d[i] == 0xFF:
            i += 1
        if i >= n:
            raise JpegError("EINVAL", "truncated header")
        m = d[i]
        i += 1
        if m == 0 or m == 1 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD8, 0xD9):
            raise JpegError("EINVAL", "SOI / EOI before a scan")
        if i + 2 > n:
            raise JpegError("EINVAL", "truncated segment")
        L = (d[i] << 8) | d[i + 1]
        if L < 2 or i + L > n:
            raise JpegError("EINVAL", "truncated segment")
        s = d[i + 2:i + L]
        i += L
        if m in (0xC0, 0xC1):
            if sof is not None or len(s) < 6:
                raise JpegError("EINVAL", "SOF")
            prec, hh, ww, nf = s[0], (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if prec == 12:
                raise JpegError("EUNSUPPORTED", "12-bit")
            if prec != 8 or ww == 0 or nf == 0 or len(s) < 6 + 3 * nf:
                raise JpegError("EINVAL", "SOF")
            if hh == 0:
                raise JpegError("EUNSUPPORTED", "DNL")
            if nf not in (1, 3):
                raise JpegError("EUNSUPPORTED", "components")
            comps = []
            for c in range(nf):
                cid, hv, tq = s[6 + 3 * c], s[7 + 3 * c], s[8 + 3 * c]
                ch, cv = hv >> 4, hv & 15
                if not (1 <= ch <= 4 and 1 <= cv <= 4) or tq > 3 or cid in [x[0] for x in comps]:
                    raise JpegError("EINVAL", "component")
                comps.append((cid, ch, cv, tq))
            if comps[0][1] > 2 or comps[0][2] > 2 or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                raise JpegError("EUNSUPPORTED", "sampling")
            sof = (hh, ww, comps)
        elif 0xC2 <= m <= 0xCF and m != 0xC4:
            raise JpegError("EUNSUPPORTED", "SOF%x" % m)
        elif m == 0xC4:
            o = 0
            while o < len(s):
                tc, th = s[o] >> 4, s[o] & 15
                if tc > 1 or th > 3 or o + 17 > len(s):
                    raise JpegError("EINVAL", "DHT")
                bits = list(s[o + 1:o + 17])
                cnt = sum(bits)
                if cnt > 256 or o + 17 + cnt > len(s):
                    raise JpegError("EINVAL", "DHT")
                vals = list(s[o + 17:o + 17 + cnt])
                code = 0
                for l in range(1, 17):
                    code += bits[l - 1]
                    if code >= (1 << l):
                        raise JpegError("EINVAL", "DHT codes")
                    code <<= 1
                if tc == 0 and any(v > 15 for v in vals):
                    raise JpegError("EINVAL", "DHT DC symbol")
                (ac if tc else dc)[th] = (bits, vals)
                o += 17 + cnt
            has_dht = True
        elif m == 0xDB:
            o = 0
            while o < len(s):
                pq, tq = s[o] >> 4, s[o] & 15
                if pq > 1 or tq > 3 or o + 1 + 64 * (pq + 1) > len(s):
                    raise JpegError("EINVAL", "DQT")
                q = np.zeros(64, np.int64)
                for k in range(64):
                    q[ZIGZAG[k]] = (s[o + 1 + 2 * k] << 8 | s[o + 2 + 2 * k]) if pq else s[o + 1 + k]
                qt[tq] = q
                o += 1 + 64 * (pq + 1)
        elif m == 0xDD:
            if len(s) != 2:
                raise JpegError("EINVAL", "DRI")
            restart = (s[0] << 8) | s[1]
        elif m == 0xDA:
            if sof is None or len(s) < 1:
                raise JpegError("EINVAL", "SOS")
            ns = s[0]
            if not 1 <= ns <= 4 or len(s) < 1 + 2 * ns + 3:
                raise JpegError("EINVAL", "SOS")
            hh, ww, comps = sof
            ids = [x[0] for x in comps]
            idx, sel = [], []
            for c in range(ns):
                cs, td, ta = s[1 + 2 * c], s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                if td > 3 or ta > 3 or cs not in ids or ids.index(cs) in idx:
                    raise JpegError("EINVAL", "SOS component")
                idx.append(ids.index(cs))
                sel.append((td, ta))
            if (s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns]) != (0, 63, 0):
                raise JpegError("EINVAL", "SOS spectral selection")
            if ns != len(comps):
                raise JpegError("EUNSUPPORTED", "non-interleaved scan")
            if idx != list(range(ns)):
                raise JpegError("EINVAL", "scan order")
            tabs = []
            for c, (td, ta) in enumerate(sel):
                if comps[c][3] not in qt:
                    raise JpegError("EINVAL", "no DQT")
                if (td not in dc and td > 1) or (ta not in ac and ta > 1):
                    raise JpegError("EINVAL", "no DHT")
                tabs.append((dc.get(td) or STD_TABLES[(0, td)], ac.get(ta) or STD_TABLES[(1, ta)]))
            return {"width": ww, "height": hh, "n_components": len(comps), "h_samp": comps[0][1], "v_samp": comps[0][2],
                    "restart_interval": restart, "has_dht": int(has_dht), "qt": qt[comps[0][3]], "tables": tabs, "scan_off": i}


# ---- decoder ----------------------------------------------------------------------------------------------------------------
def _lut16(bits, vals):
    """(length << 8 | symbol) of the code each 16-bit window starts with; 0 = no code."""
    lut = np.zeros(65536, np.int64)
    for sym, (code, l) in _codes(bits, vals).items():
        lut[code << (16 - l):(code + 1) << (16 - l)] = (l << 8) | sym
    return lut.tolist()


def unstuff(scan):
    """(unstuffed bytes, [(offset in them, RST number)]) up to the first marker that is not RSTn."""
    out, rst = bytearray(), []
    n, i = len(scan), 0
    while i < n:
        b = scan[i]
        if b != 0xFF:
            out.append(b)
            i += 1
            continue
        j = i
        while j < n and scan[j] == 0xFF:
            j += 1
        if j >= n:
            break
        if scan[j] == 0:
            out.append(0xFF)
            i = j + 1
        elif 0xD0 <= scan[j] <= 0xD7:
            rst.append((len(out), scan[j] - 0xD0))
            i = j + 1
        else:
            break
    return bytes(out), rst


def _range_limit(x):
    j = x.astype(np.int64) & 1023
    return np.where(j < 128, j + 128, np.where(j < 512, 255, np.where(j < 896, 0, j - 896))).astype(np.uint8)


def _islow_1d(v):
    """jpeg_idct_islow's 1-D pass along the last axis on int64, before descaling."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (v[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    tmp2 = z1 + i6 * -15137
    tmp3 = z1 + i2 * 6270
    tmp0 = (i0 + i4) * 8192
    tmp1 = (i0 - i4) * 8192
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i7, i5, i3, i1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([t10 + tmp3, t11 + tmp2, t12 + tmp1, t13 + tmp0, t13 - tmp0, t12 - tmp1, t11 - tmp2, t10 - tmp3], axis=-1)


def idct_islow(coef, q):
    """coef [n][64] natural order (int16 values), q [64] -> [n][8][8] uint8: libjpeg-turbo's jpeg_idct_islow with its range limit
    (the index into the table is masked, so out-of-range values wrap as libjpeg's do)."""
    dq = np.asarray(coef, np.int64).reshape(-1, 8, 8) * np.asarray(q, np.int64).reshape(8, 8)
    cols = _islow_1d(dq.transpose(0, 2, 1))                            # [n][column][row]
    ws = ((cols + 1024) >> 11).astype(np.int32).transpose(0, 2, 1)    # the int workspace, [n][row][column]
    rows = _islow_1d(ws.astype(np.int64))
    return _range_limit((rows + (1 << 17)) >> 18)


def decode_luma(data, info=None):
    """(luma [h][w] uint8, status) under the library's rules; a frame that fails is all zeros ([0][0] when the header is
    refused).  info: a dict that receives "end_bits", the bit position in the unstuffed scan after the last block of every
    interval that was decoded whole (tests/jpeg_sync_model.py is checked against it)."""
    try:
        P = parse(data)
    except JpegError as e:
        return np.zeros((0, 0), np.uint8), (UNSUPPORTED if e.code == "EUNSUPPORTED" else CORRUPT)
    w, h, nc = P["width"], P["height"], P["n_components"]
    H, V = (P["h_samp"], P["v_samp"]) if nc == 3 else (1, 1)
    nyb = H * V
    bpm = nyb + 2 if nc == 3 else 1
    mcux, mcuy = -(-w // (8 * H)), -(-h // (8 * V))
    nmcu = mcux * mcuy
    R = P["restart_interval"] or nmcu
    nint = -(-nmcu // R)
    zero = np.zeros((h, w), np.uint8)
    comp, rst = unstuff(bytes(data)[P["scan_off"]:])
    if len(rst) != nint - 1 or any(r != (k & 7) for k, (_, r) in enumerate(rst)):
        return zero, CORRUPT
    starts = [0] + [o for o, _ in rst] + [len(comp)]
    c = np.frombuffer(comp + b"\xff" * 8, np.uint8).astype(np.int64)
    win = ((c[:-3] << 24) | (c[1:-2] << 16) | (c[2:-1] << 8) | c[3:]).tolist()
    far = len(comp) * 8 + 32

    def peek(p, nbits):   # bits past the scan read as ones
        if p >= far:
            return (1 << nbits) - 1
        return ((win[p >> 3] << (p & 7)) & 0xFFFFFFFF) >> (32 - nbits)
    luts = [(_lut16(*dct), _lut16(*act)) for dct, act in P["tables"]]
    nat = ZIGZAG.tolist()
    ycoef = [[0] * 64 for _ in range(mcuy * V * mcux * H)]
    ystride = mcux * H
    for k in range(nint):
        pos, lim = starts[k] * 8, starts[k + 1] * 8
        last = [0, 0, 0]
        for b in range(min(R, nmcu - k * R) * bpm):
            mcu, sl = k * R + b // bpm, b % bpm
            ci = 0 if sl < nyb else sl - nyb + 1
            dcl, acl = luts[ci]
            if ci == 0:
                my, mx = divmod(mcu, mcux)
                blk = ycoef[(my * V + sl // H) * ystride + mx * H + sl % H]
            else:
                blk = [0] * 64
            e = dcl[peek(pos, 16)]
            if not e:
                return zero, CORRUPT
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
                    return zero, CORRUPT
                pos += e >> 8
                r, s = (e & 255) >> 4, e & 15
                if s:
                    kk += r
                    if kk > 63:
                        return zero, CORRUPT
                    v = peek(pos, s)
                    pos += s
                    blk[nat[kk]] = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                    kk += 1
                elif r == 15:
                    if kk + 15 > 63:
                        return zero, CORRUPT
                    kk += 16
                else:
                    break
            if pos > lim:     # the interval ends before its MCUs do
                return zero, CORRUPT
        if info is not None:
            info.setdefault("end_bits", []).append(pos)
    yc = np.array(ycoef, np.int64)
    yc = (yc + 32768) % 65536 - 32768                               # libjpeg stores coefficients as 16-bit JCOEFs
    pix = idct_islow(yc, P["qt"]).reshape(mcuy * V, mcux * H, 8, 8).transpose(0, 2, 1, 3).reshape(mcuy * V * 8, mcux * H * 8)
    return np.ascontiguousarray(pix[:h, :w]), OK
