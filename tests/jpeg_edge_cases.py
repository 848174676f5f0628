"""Named JPEG streams that put k_jpeg_frame (chalkydri_amd/csrc/k_jpeg.hip) at its own edges, each with the
conditions it has to meet.  The conditions are figures of tests/jpeg_sync_model.py (which path the synchronisation takes, stale
and empty pieces, the cap, ...) or byte offsets read from the stream itself; measure(name) asserts them on the CPU and returns what
tests/np_jpeg.py decodes, which is what the device has to give.  A family is one batch: all its streams have the family's size.
No case is skipped or dropped at run time: a case that stops meeting a condition fails, naming the figure."""
import functools
import operator

import numpy as np

import jpeg_sync_model as M
import np_jpeg as J

K = M.constants()
SUB, ROUNDS, MAXB, NT = K["SUB_BITS"], K["SYNC_ROUNDS"], K["MAX_BLOCK_BYTES"], K["FRAME_THREADS"]
SAMPLINGS = ("444", "422", "440", "420", "grey")
SIZES = {"paths": (96, 64), "periodic": (264, 264), "pieces": (264, 264), "tails": (48, 32), "short": (48, 32), "unstuff": (48, 32),
         "scans": (264, 264), "symbols": (48, 32)}   # width x height of every stream of the family
FAMILIES = tuple(SIZES)
OPS = {"==": operator.eq, ">=": operator.ge, ">": operator.gt, "<=": operator.le, "<": operator.lt, "!=": operator.ne,
       "has": lambda a, b: b in a}


def cond(key, op, value):
    """(label, test on the figures): figure `key` `op` value ("has": value is among the figure's entries)"""
    return "%s %s %r" % (key, op, value), lambda fig: OPS[op](fig[key], value)


def where(label, fn):
    return label, fn


OK_BLOCKS = where("status == OK with every interval's blocks", lambda fig: fig["status"] == J.OK and fig["blocks"] == fig["need"])
IS_CORRUPT = cond("status", "==", J.CORRUPT)


# ---- content ------------------------------------------------------------------------------------------------------------------
def flat(w, h, v=77):
    return np.full((h, w), v, np.uint8)


def ramp(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(xx * 2 + yy, 0, 255).astype(np.uint8)


def stripes(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx // 3) % 2) * 200 + 20).astype(np.uint8)


def noise(w, h, seed=1):
    return (np.random.default_rng(seed).random((h, w)) * 256).astype(np.uint8)


def patched(w, h, rows, seed=1, base=77):
    """flat, with noise in the rows [rows[0], rows[1])"""
    img = flat(w, h, base)
    img[rows[0]:rows[1]] = noise(w, h, seed)[rows[0]:rows[1]]
    return img


def from_coefs(w, h, quality, block):
    """An image whose 8x8 blocks quantise (table 0 at `quality`) to block(i) [64] in zig-zag order, i in raster order; the values
    have to be coarse enough to survive the rounding of the samples (the cases' conditions check what came out)."""
    qt = J.quant_table(quality, 0).astype(np.float64)
    img = np.zeros((h, w), np.float64)
    for by in range(h // 8):
        for bx in range(w // 8):
            z = np.zeros(64)
            z[J.ZIGZAG] = np.asarray(block(by * (w // 8) + bx), np.float64)
            img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = J._C8.T @ (z * qt).reshape(8, 8) @ J._C8 + 128
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


# ---- bytes between an interval's last block and the next marker --------------------------------------------------------------
def junk(kind, n, seed=0, table=J.STD_TABLES[(1, 0)]):
    """n bytes of the unstuffed scan (raw: twice as many for "ones"), free of markers"""
    if kind == "zeros":
        return bytes(n)
    if kind == "random":      # no 0xFF at all: what is appended is what is unstuffed
        return np.random.default_rng(seed).integers(0, 255, n, dtype=np.uint8).tobytes()
    if kind == "ones":        # sixteen 1-bits are never a code
        return b"\xff\x00" * n
    assert kind == "runpast"  # DC category 0, then (run 15, size 1) five times: the fifth passes coefficient 63
    ac, dc = J._codes(*table), J._codes(*J.STD_TABLES[(0, 0)])
    vals, lens = [dc[0][0]], [dc[0][1]]
    for _ in range(5):
        vals += [ac[0xF1][0], 0]
        lens += [ac[0xF1][1], 1]
    total = sum(lens)
    reps = -(-n * 8 // total)
    return J.stuff(J.pack_bits(vals * reps, lens * reps)[:n])


def raw_scan(b):
    return bytes(b)[J.parse(b)["scan_off"]:]


def marker_offsets(b):
    """offsets in the raw scan of the 0xFF of every RSTn, then of the terminating marker"""
    raw = raw_scan(b)
    out, i = [], 0
    while i + 1 < len(raw):
        if raw[i] == 0xFF and raw[i + 1] not in (0x00, 0xFF):
            out.append(i)
            if not 0xD0 <= raw[i + 1] <= 0xD7:
                return out
            i += 1
        i += 1
    return out


def case(name, data, *conds, libjpeg=None):
    """libjpeg: whether Pillow's decode is compared (default: when the expected status is OK)"""
    return {"name": name, "data": bytes(data), "conds": list(conds), "libjpeg": libjpeg}


# ---- the families ---------------------------------------------------------------------------------------------------------------
def _paths():
    w, h = SIZES["paths"]
    E = J.encode
    out = []
    for cname, img, q in (("flat", flat(w, h), 85), ("ramp", ramp(w, h), 85), ("stripes", stripes(w, h), 85), ("noise", noise(w, h), 100)):
        for s in SAMPLINGS:
            out.append(case("grid_%s_%s" % (cname, s), E(img, sampling=s, quality=q), OK_BLOCKS))
    settled = cond("path", "==", "settled")
    out += [case("rounds0", E(flat(w, h), sampling="grey", quality=100), OK_BLOCKS, cond("frame_rounds", "==", 0), settled, cond("pieces", ">", 1)),
            case("rounds1", E(ramp(w, h), sampling="grey", quality=85), OK_BLOCKS, cond("frame_rounds", "==", 1), settled),
            case("rounds2", E(ramp(w, h), sampling="444", quality=85), OK_BLOCKS, cond("frame_rounds", "==", 2), settled),
            case("rounds3", E(ramp(w, h), sampling="420", quality=85), OK_BLOCKS, cond("frame_rounds", "==", 3), settled),
            case("rounds_exact", E(ramp(w, h), sampling="422", quality=85), OK_BLOCKS, cond("frame_rounds", "==", ROUNDS),
                 cond("path", "==", "walk"), cond("walk_redecoded", "==", 0)),
            case("rounds_beyond", E(noise(w, h), sampling="444", quality=100), OK_BLOCKS, cond("frame_rounds", ">=", 8 * ROUNDS),
                 cond("path", "==", "walk"), cond("walk_redecoded", ">=", 100))]
    half = ramp(w, h)
    half[h // 2:] = noise(w, h, 5)[h // 2:]
    for s, dri in (("420", 3), ("grey", 24)):
        out.append(case("dri_mixed_" + s, E(half, sampling=s, quality=100, restart_interval=dri), OK_BLOCKS, cond("path", "==", "walk"),
                        where("intervals below and above SYNC_ROUNDS", lambda f: min(f["rounds"]) < ROUNDS < max(f["rounds"])),
                        cond("walk_redecoded", ">", 0)))
    return out


def _periodic():
    w, h = SIZES["periodic"]
    out = []
    for level in (0, 128, 255, 77):
        for s in SAMPLINGS:
            for dri in (0, 7):
                chroma = None if s == "grey" else (flat(w, h, 128), flat(w, h, 128))
                conds = [OK_BLOCKS, cond("pieces", ">", 1)]
                if level == 128 and dri == 0:   # every MCU of the frame is the same bits: 6 for grey, 14 / 20 / 20 / 32 with chroma
                    mcu_bits = {"grey": 6, "444": 14, "422": 20, "440": 20, "420": 32}[s]
                    if SUB % mcu_bits == 0:
                        conds.append(where("every piece starts an MCU", lambda f: f["mcu_aligned_pieces"] == f["pieces"] - 1))
                    else:
                        conds.append(where("piece starts on and off MCU boundaries", lambda f: 0 < f["mcu_aligned_pieces"] < f["pieces"] - 1))
                out.append(case("level%d_%s_dri%d" % (level, s, dri), J.encode(flat(w, h, level), sampling=s, quality=85, restart_interval=dri,
                                                                             chroma=chroma), *conds))
    return out


def _padded(make, k, nbytes):
    """make(append) with interval k padded by zeros to nbytes of unstuffed scan"""
    have = M.run(make(append=None))["interval_bytes"][k]
    assert have <= nbytes, (have, nbytes)
    return make(append={k: bytes(nbytes - have)})


def _pieces():
    w, h = SIZES["pieces"]
    busy = patched(w, h, (h - 16, h), seed=3)
    row = lambda append=None: J.encode(flat(w, h, 90), sampling="grey", quality=85, restart_interval=33, append=append)  # noqa: E731
    in5 = lambda f: f["last_piece"][5] - f["first_piece"][5] + 1  # noqa: E731
    return [
        case("many_intervals", J.encode(busy, sampling="444", quality=100, restart_interval=1), OK_BLOCKS, cond("intervals", ">", NT),
             cond("pieces", ">", NT + 64), where("an interval shorter than a piece", lambda f: 0 < min(f["interval_bytes"]) * 8 < SUB),
             cond("spanning_blocks", ">", 0), cond("zero_block_pieces", ">", 0)),
        case("short_intervals", row(), OK_BLOCKS, where("every interval shorter than a piece", lambda f: max(f["interval_bytes"]) * 8 < SUB),
             cond("pieces", "==", 33)),
        case("one_piece_exactly", _padded(row, 5, SUB // 8), OK_BLOCKS, where("interval 5 is SUB bits", lambda f: f["interval_bytes"][5] * 8 == SUB),
             where("... one piece", lambda f: in5(f) == 1)),
        case("one_piece_and_a_byte", _padded(row, 5, SUB // 8 + 1), OK_BLOCKS,
             where("interval 5 is SUB + 8 bits", lambda f: f["interval_bytes"][5] * 8 == SUB + 8), where("... two pieces", lambda f: in5(f) == 2)),
        case("one_byte_short_of_a_piece", _padded(row, 5, SUB // 8 - 1), OK_BLOCKS, where("... one piece", lambda f: in5(f) == 1)),
        case("spanning_grey", J.encode(patched(w, h, (64, 96), seed=4), sampling="grey", quality=100), OK_BLOCKS, cond("spanning_blocks", ">", 0),
             cond("zero_block_pieces", ">", 0), cond("code_straddles", ">", 0), cond("field_straddles", ">", 0), cond("path", "==", "walk")),
        case("spanning_420_rows", J.encode(patched(w, h, (128, 160), seed=5), sampling="420", quality=100, restart_interval=1, restart_rows=True),
             OK_BLOCKS, cond("spanning_blocks", ">", 0), cond("zero_block_pieces", ">", 0), cond("code_straddles", ">", 0),
             cond("field_straddles", ">", 0)),
    ]


def _tail_bases():
    w, h = SIZES["tails"]
    img = noise(w, h, 7)
    return {"grey": functools.partial(J.encode, img, sampling="grey", quality=95, restart_interval=2),        # 12 intervals of 2 blocks
            "g100": functools.partial(J.encode, img, sampling="grey", quality=100, restart_interval=6),       # 4 intervals, the walk
            "420": functools.partial(J.encode, img, sampling="420", quality=95)}                              # one interval of 36 blocks


def _tails():
    B = _tail_bases()
    out = []
    seen = {"ones": cond("tail_invalid", ">", 0), "runpast": cond("tail_runpast", ">", 0)}
    for kind in ("zeros", "random", "ones", "runpast"):
        extra = [seen[kind]] if kind in seen else []
        out.append(case("last_%s_one_piece" % kind, B["grey"](append={-1: junk(kind, SUB // 8)}), OK_BLOCKS, *extra))
        out.append(case("middle_%s_pieces" % kind, B["grey"](append={3: junk(kind, 5 * SUB // 8 + 3, 1)}), OK_BLOCKS, *extra))
        out.append(case("last_%s_420" % kind, B["420"](append={-1: junk(kind, 3 * SUB // 8 + 1, 2)}), OK_BLOCKS))
    for d in (-1, 0, 1):   # interval 4 needs 2 blocks
        out.append(case("cap%+d" % d, _padded(B["grey"], 4, 2 * MAXB + d), OK_BLOCKS,
                        where("interval 4 is 2 * MAX_BLOCK_BYTES %+d bytes" % d, lambda f, d=d: f["interval_bytes"][4] == 2 * MAXB + d),
                        cond("cap_cut", "==", 1 if d > 0 else 0)))
        out.append(case("cap%+d_last" % d, _padded(B["grey"], 11, 2 * MAXB + d), OK_BLOCKS,
                        where("the last interval is 2 * MAX_BLOCK_BYTES %+d bytes" % d, lambda f, d=d: f["interval_bytes"][11] == 2 * MAXB + d),
                        cond("cap_cut", "==", 1 if d > 0 else 0)))
    out.append(case("cap_far_420", B["420"](append={-1: junk("random", 36 * MAXB + 2000, 3)}), OK_BLOCKS, cond("cap_cut", "==", 1)))
    out.append(case("fill_before_rst", B["grey"](fill={3: 3, 7: 1}), OK_BLOCKS))
    out.append(case("fill_before_eoi", B["grey"](fill={-1: 2}), OK_BLOCKS))
    out.append(case("fill_and_junk", B["grey"](append={5: junk("random", 70, 4)}, fill={5: 2, -1: 5}), OK_BLOCKS))
    out.append(case("after_eoi", B["grey"]() + b"\xff\xd0\xff\xd1\x12\xff\x00\x34\xff\xd2\xff\xd9\xff\xff\xd3\x00", OK_BLOCKS))
    out.append(case("after_eoi_420", B["420"](append={-1: junk("zeros", 9)}) + b"\xff\x00\xff\xd0" * 40, OK_BLOCKS))
    for seed in (1, 2):
        kind = ("zeros", "runpast")[seed - 1]
        out.append(case("stale_" + kind, B["g100"](append={1: junk(kind, 40 * SUB // 8), -1: junk(kind, 30 * SUB // 8)}),
                        OK_BLOCKS, cond("path", "==", "walk"), cond("walk_stale", ">", 0), cond("walk_skipped", ">", 0)))
    return out


def _cut(b, k, nbytes):
    """the stream with the last nbytes raw bytes of interval k removed (in front of the marker that ends it)"""
    off = J.parse(b)["scan_off"]
    end = off + marker_offsets(b)[k]
    return b[:end - nbytes] + b[end:]


def _keep(b, k, nbytes):
    """the stream with interval k cut after nbytes bytes of its unstuffed scan"""
    off, mo = J.parse(b)["scan_off"], marker_offsets(b)
    i, end = off + (mo[k - 1] + 2 if k else 0), off + mo[k]
    for _ in range(nbytes):
        i += 2 if b[i] == 0xFF else 1
    assert i <= end
    return b[:i] + b[end:]


def _insert(b, k, extra):
    """the stream with `extra` in front of the marker that ends interval k"""
    at = J.parse(b)["scan_off"] + marker_offsets(b)[k]
    return b[:at] + extra + b[at:]


def _short():
    B = _tail_bases()
    good = [B["grey"](), B["420"](), B["g100"]()]
    base = B["grey"]()
    out = []

    def bad(name, data, *conds):
        out.append(case(name, data, IS_CORRUPT, *conds))
        out.append(case("good_after_" + name, good[len(out) % 3], OK_BLOCKS))
    out.append(case("good_first", good[0], OK_BLOCKS))
    short = cond("short_intervals", ">", 0)
    # the last block of an interval ends in its last byte (the padding is less than a byte): one byte less cuts it
    bad("middle_cut", _cut(base, 3, 1), short)
    bad("last_cut", _cut(base, 11, 1), short)
    bad("middle_cut_fill", _insert(_cut(base, 3, 1), 3, b"\xff" * 3), short)
    bad("last_cut_fill", _insert(_cut(base, 11, 1), 11, b"\xff" * 2), short)
    bad("last_cut_after_eoi", _cut(base, 11, 1) + b"\xff\xd3\xff\x00\x55\xff\xd9", short)
    bad("last_cut_ones", _insert(_cut(base, 11, 1), 11, junk("ones", 40)))      # the cut block runs into an invalid code
    # ... and into bytes that complete it: whatever np_jpeg (and libjpeg) make of these bits is what the device has to give
    out.append(case("middle_cut_zeros", _insert(_cut(base, 3, 1), 3, bytes(64))))
    out.append(case("middle_cut_runpast", _insert(_cut(base, 3, 1), 3, junk("runpast", 64))))
    bad("cut_420", _cut(B["420"](), 0, 2), short)
    bad("cut_420_after_eoi", _cut(B["420"](), 0, 1) + bytes(50) + b"\xff\xd0", short)
    mo = marker_offsets(base)
    bad("empty_interval", _cut(base, 6, mo[6] - mo[5] - 2), short,
        where("interval 6 is empty: its block starts at the limit", lambda f: f["interval_bytes"][6] == 0))
    # an interval whose first block ends on a byte boundary, cut there: the second block it needs starts exactly at the limit
    aligned = None
    for seed in range(64):
        b = J.encode(noise(48, 32, 100 + seed), sampling="grey", quality=95, restart_interval=2)
        f = M.run(b)
        ks = [k for k in range(1, 11) if f["first_block_end"][k] % 8 == 0]
        if ks:
            k = ks[0]
            keep = f["first_block_end"][k] // 8 - f["interval_start"][k]
            aligned = (_keep(b, k, keep), k, keep)
            break
    assert aligned, "no interval whose first block ends on a byte boundary"
    data, k, keep = aligned
    bad("block_starts_at_the_limit", data, short,
        where("interval %d ends where its second block starts" % k, lambda f: f["interval_bytes"][k] == keep and f["blocks"][k] == 1))
    return out


def _unstuff():
    w, h = SIZES["unstuff"]
    img = noise(w, h, 9)
    img[:8, :16] = 60                       # interval 0 (two blocks) is a few bytes
    E = functools.partial(J.encode, img, sampling="grey", quality=95, restart_interval=2)
    plain = E()
    len0, total = marker_offsets(plain)[0], marker_offsets(plain)[-1]
    out = []

    def at(name, data, i, pair, m, *conds):
        raw = raw_scan(data)
        assert raw[i:i + 2] == pair and i % m == m - 1, (name, i, raw[i:i + 2].hex(), m)
        out.append(case(name, data, OK_BLOCKS, where("bytes %s at raw offsets %d | %d" % (pair.hex(), i, i + 1),
                                                      lambda f: raw_scan(data)[i:i + 2] == pair and i % m == m - 1), *conds))
    for m, tag in ((4, "lane"), (256, "wave"), (4 * NT, "chunk")):
        i = next(x for x in range(len0 + 1, 3 * 4 * NT) if x % m == m - 1)
        at("ff00_" + tag, E(append={0: junk("random", i - len0, m) + b"\xff\x00" + junk("random", 6, m + 1)}), i, b"\xff\x00", m)
        at("rst_" + tag, E(append={0: junk("random", i - len0, m + 2)}), i, b"\xff\xd0", m)
        at("fill_" + tag, E(append={0: junk("random", i - len0, m + 3)}, fill={0: 2}), i, b"\xff\xff", m)
        at("fill_rst_" + tag, E(append={0: junk("random", i - 1 - len0, m + 4)}, fill={0: 1}), i, b"\xff\xd0", m)
        j = next(x for x in range(total + 1, 3 * 4 * NT) if x % m == m - 1)
        at("eoi_" + tag, E(append={-1: junk("random", j - total, m + 5)}) + b"\xff\xd0\xff\x00", j, b"\xff\xd9", m)
    # a stuffed byte of the scan's own, not of the padding: the first FF 00 of a q100 noise stream moved onto a lane, wave and chunk boundary
    hot = functools.partial(J.encode, noise(w, h, 11), sampling="grey", quality=100, restart_interval=6)
    first_rst = marker_offsets(hot())[0]
    pos = raw_scan(hot()).index(b"\xff\x00", first_rst)   # (after interval 0, which takes the padding)
    for m, tag in ((4, "lane"), (256, "wave"), (4 * NT, "chunk")):
        pad = next(x for x in range(0, 2 * m) if (pos + x) % m == m - 1)
        at("own_ff00_" + tag, hot(append={0: junk("random", pad, 30 + m)}), pos + pad, b"\xff\x00", m)
    for r in (3, 0, 1):
        n = next(x for x in range(4) if (M.run(plain)["unstuffed_bytes"] + x) % 4 == r)
        out.append(case("length_4k%+d" % (r if r < 2 else -1), E(append={-1: junk("random", n, 40 + r)}), OK_BLOCKS,
                        where("unstuffed length %% 4 == %d" % r, lambda f, r=r: f["unstuffed_bytes"] % 4 == r)))
    hot_b = hot()
    cut = J.parse(hot_b)["scan_off"] + pos + 1
    out.append(case("truncated_after_ff", hot_b[:cut], IS_CORRUPT, where("the payload ends in FF", lambda f: hot_b[cut - 1] == 0xFF), libjpeg=False))
    one = J.encode(noise(w, h, 11), sampling="grey", quality=100)
    cut1 = J.parse(one)["scan_off"] + raw_scan(one).index(b"\xff\x00", 600) + 1
    out.append(case("truncated_after_ff_one_interval", one[:cut1], IS_CORRUPT, cond("short_intervals", "==", 1),
                    where("the payload ends in FF", lambda f: one[cut1 - 1] == 0xFF), libjpeg=False))
    out.append(case("eoi_half", plain[:-1], OK_BLOCKS, where("the payload ends in FF", lambda f: plain[-2] == 0xFF), libjpeg=False))
    return out


def dc_wrap_stream(w, h, dri):
    """A grey stream whose every block is one DC difference of +-2047 and EOB: the running sum passes +-32767 again and again."""
    tmpl = J.encode(flat(w, h), sampling="grey", quality=50, restart_interval=dri)
    head = tmpl[:J.parse(tmpl)["scan_off"]]
    dc, ac = J._codes(*J.STD_TABLES[(0, 0)]), J._codes(*J.STD_TABLES[(1, 0)])
    nblk = -(-w // 8) * -(-h // 8)
    R = dri or nblk
    scan, peak = bytearray(), 0
    for k in range(-(-nblk // R)):
        vals, lens, run = [], [], 0
        for b in range(min(R, nblk - k * R)):
            d = 2047 if (b // 45) % 3 != 1 else -2047
            run += d
            peak = max(peak, abs(run))
            vals += [dc[11][0], d if d > 0 else d + 2047, ac[0][0]]
            lens += [dc[11][1], 11, ac[0][1]]
        if k:
            scan += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        scan += J.stuff(J.pack_bits(vals, lens))
    assert peak > 2 * 32768, peak
    return head + bytes(scan) + b"\xff\xd9"


def _scans():
    w, h = SIZES["scans"]
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.clip(128 + 90 * np.sin(xx / 19.0) * np.cos(yy / 13.0) + 20 * ((xx // 31 + yy // 17) % 2), 0, 255).astype(np.uint8)
    offs = np.where((np.arange(1200) // 7) % 2 == 0, 60, -60)   # (samples stay where libjpeg's range limit clamps: its SIMD IDCT equals the C code there, §4c)
    out = [case("grey_one_interval", J.encode(smooth, sampling="grey", quality=50), OK_BLOCKS, where("more Y blocks than threads", lambda f: f["need"][0] > NT)),
           case("420_one_interval", J.encode(smooth, sampling="420", quality=50), OK_BLOCKS, where("more Y blocks than threads", lambda f: f["need"][0] * 4 // 6 > NT)),
           case("grey_dc_offsets", J.encode(smooth, sampling="grey", quality=50, dc_offset=offs), OK_BLOCKS)]
    for t, dri in ((NT - 1, (NT - 1) // 3), (NT, NT // 4), (NT + 1, (NT + 1) // 5)):
        assert t % dri == 0
        for s in ("grey", "444"):
            out.append(case("%s_interval_at_t%d" % (s, t), J.encode(smooth, sampling=s, quality=50, restart_interval=dri, dc_offset=offs), OK_BLOCKS,
                            cond("dc_index", "has", t)))
    out.append(case("420_interval_at_t%d" % NT, J.encode(smooth, sampling="420", quality=50, restart_interval=NT // 4), OK_BLOCKS, cond("dc_index", "has", NT)))
    # block-index pass: ~1000 one-piece intervals, then intervals of several pieces across s = NT; padding interval 2 shifts them
    busy = patched(w, h, (h - 24, h), seed=6)
    make = lambda n: J.encode(busy, sampling="444", quality=100, restart_interval=1, append={2: junk("random", n * SUB // 8, 50)} if n else None)  # noqa: E731
    f0 = M.run(make(0))
    x = max(b for a, b in zip(f0["first_piece"], f0["last_piece"]) if b - a >= 2 and b <= NT - 1)   # an interval of three pieces or more
    for s in (NT - 1, NT, NT + 1):
        edge = where("the next interval starts at s = %d" % NT, lambda f: NT in f["first_piece"]) if s == NT - 1 else \
            where("the interval's pieces lie on both sides of s = %d | %d" % (NT - 1, NT),
                  lambda f, s=s: f["first_piece"][f["last_piece"].index(s)] <= NT - 1)
        out.append(case("last_piece_at_s%d" % s, make(s - x), OK_BLOCKS, cond("last_piece", "has", s), edge))
    # (not compared with Pillow: wrapped DCs are outside the range in which libjpeg-turbo's SIMD IDCT equals the C code, §4c)
    out.append(case("dc_wrap", dc_wrap_stream(w, h, 0), OK_BLOCKS, libjpeg=False))
    out.append(case("dc_wrap_dri", dc_wrap_stream(w, h, (NT + 1) // 5), OK_BLOCKS, cond("dc_index", "has", NT + 1), libjpeg=False))
    return out


DC16 = ([0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0])   # the common categories get the 14- to 16-bit codes


def _symbols():
    w, h = SIZES["symbols"]
    rng = np.random.default_rng(12)
    long_tables = {(0, 0): DC16, (0, 1): DC16, (1, 0): J.shuffled_table(1, 0, rng), (1, 1): J.shuffled_table(1, 1, rng)}
    eob_tables = {(1, t): (list(J.STD_TABLES[(1, t)][0]), [0x10 + 0x10 * t if v == 0xFA else v for v in J.STD_TABLES[(1, t)][1]]) for t in (0, 1)}
    zrl3 = from_coefs(w, h, 50, lambda i: [i % 5 - 2] + [0] * 62 + [2 if i % 2 else -3])
    sgn = np.where(np.random.default_rng(13).random((24, 63)) < 0.5, -2, 2)
    full = from_coefs(w, h, 90, lambda i: [0] + list(sgn[i]))
    out = []
    for s in ("grey", "420", "444"):
        out.append(case("codes16_" + s, J.encode(noise(w, h, 14), sampling=s, quality=90, tables=long_tables, restart_interval=5 if s == "420" else 0),
                        OK_BLOCKS, cond("codes16", ">", 0), cond("long_codes", ">", 20)))
        out.append(case("eob_run_" + s, J.encode(noise(w, h, 15), sampling=s, quality=60, tables=eob_tables, eob=0x10 if s != "444" else 0x20),
                        OK_BLOCKS, cond("eob_run_syms", ">", 0)))
    out.append(case("three_zrl", J.encode(zrl3, sampling="grey", quality=50), OK_BLOCKS, cond("max_zrl", "==", 3)))
    out.append(case("three_zrl_422", J.encode(zrl3, sampling="422", quality=50, restart_interval=2), OK_BLOCKS, cond("max_zrl", "==", 3)))
    out.append(case("no_eob", J.encode(full, sampling="grey", quality=90), OK_BLOCKS, cond("no_eob_blocks", ">=", 20)))
    out.append(case("no_eob_440", J.encode(full, sampling="440", quality=90, restart_interval=1), OK_BLOCKS, cond("no_eob_blocks", ">=", 20)))
    return out


_BUILDERS = {"paths": _paths, "periodic": _periodic, "pieces": _pieces, "tails": _tails, "short": _short, "unstuff": _unstuff,
             "scans": _scans, "symbols": _symbols}


@functools.lru_cache(maxsize=None)
def family(name):
    """The cases of a family, in batch order (built once)."""
    cases = _BUILDERS[name]()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names), names
    return tuple(cases)


def names(fam):
    return ["%s/%s" % (fam, c["name"]) for c in family(fam)]


@functools.lru_cache(maxsize=None)
def measure(name):
    """name = "family/case": the model and np_jpeg.decode_luma run once; the case's conditions asserted, naming the figure.
    -> {"data", "luma" [h][w], "status", "fig", "end_bits" (np_jpeg's), "libjpeg"}"""
    fam, cname = name.split("/")
    c = next(x for x in family(fam) if x["name"] == cname)
    w, h = SIZES[fam]
    info = {}
    luma, status = J.decode_luma(c["data"], info)
    assert luma.shape == (h, w), (name, luma.shape)
    fig = M.run(c["data"])
    if "refused" in fig:
        assert fig["refused"] == status, (name, fig, status)
        fig = dict(fig, need=[], blocks=None)
    fig["status"] = status
    for label, test in c["conds"]:
        assert test(fig), "%s does not meet its condition: %s (figures: %s)" % (name, label, {k: v for k, v in fig.items()
                                                                                              if not isinstance(v, list) or len(v) < 16})
    luma.setflags(write=False)
    return {"data": c["data"], "luma": luma, "status": status, "fig": fig, "end_bits": info.get("end_bits", []),
            "libjpeg": status == J.OK if c["libjpeg"] is None else c["libjpeg"]}


def batch(fam):
    """(streams, expected luma [n][h][w], expected status words) of a family"""
    ms = [measure(n) for n in names(fam)]
    return [m["data"] for m in ms], np.stack([m["luma"] for m in ms]), [m["status"] for m in ms]
