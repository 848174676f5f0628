"""Baseline JPEG, host side (no GPU): the numpy reference decoder (tests/np_jpeg.py) against Pillow's libjpeg, the numpy encoder's
streams through Pillow, and ck_jpeg_info (the library's header parse) against both, including one refusal per rule."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg as J  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

try:
    from PIL import Image
except ImportError:   # the numpy-only checks below still run
    Image = None

needs_pil = pytest.mark.skipif(Image is None, reason="Pillow is not importable")


def pil_luma(b):
    """What libjpeg returns for a grayscale decode of the stream (GStreamer's jpegdec -> GRAY8 does the same)."""
    im = Image.open(io.BytesIO(b))
    im.draft("L", im.size)
    return np.asarray(im.convert("L"))


def pil_stream(rng, i):
    """One random Pillow-encoded stream: q 1..100, every sampling + grey, restart markers by blocks / rows, optimised tables,
    DHT stripped."""
    w, h = int(rng.integers(8, 72)), int(rng.integers(8, 72))
    if i % 3 == 0:
        img = (rng.random((h, w, 3)) * 255).astype(np.uint8)                       # noise: long codes, large coefficients
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 7 + yy * 3) % 256, (yy * 5) % 256, (xx * yy) % 256], -1).astype(np.uint8)
        img = np.clip(img.astype(int) + rng.integers(-20, 20, img.shape), 0, 255).astype(np.uint8)
    kw = {"quality": int(rng.integers(1, 101))}
    grey = i % 5 == 4
    if not grey:
        kw["subsampling"] = [0, 1, 2, "4:4:0"][i % 4]
    kind = i % 6
    if kind == 1:
        kw["restart_marker_blocks"] = int(rng.integers(1, 9))
    elif kind == 2:
        kw["restart_marker_rows"] = int(rng.integers(1, 4))
    elif kind == 3:
        kw["optimize"] = True
    buf = io.BytesIO()
    try:
        Image.fromarray(img[..., 0] if grey else img).save(buf, "JPEG", **kw)
    except (ValueError, KeyError, TypeError):          # an older Pillow without 4:4:0 / restart options: fall back to defaults
        buf = io.BytesIO()
        Image.fromarray(img[..., 0] if grey else img).save(buf, "JPEG", quality=kw["quality"])
    b = buf.getvalue()
    if kind == 4:
        b = J.strip_dht(b)
    return b


def lib_info(b):
    from chalkydri_amd.detector import jpeg_info
    from chalkydri_amd._lib import ChalkydriError
    try:
        return A.CK_OK, jpeg_info(b)
    except ChalkydriError as e:
        return e.code, None


def np_info(b):
    try:
        p = J.parse(b)
    except J.JpegError as e:
        return {"EINVAL": A.CK_EINVAL, "EUNSUPPORTED": A.CK_EUNSUPPORTED}[e.code], None
    return A.CK_OK, {k: p[k] for k in ("width", "height", "n_components", "h_samp", "v_samp", "restart_interval", "has_dht")}


@needs_pil
def test_numpy_decoder_equals_libjpeg_on_pillow_streams():
    rng = np.random.default_rng(2024)
    for i in range(240):
        b = pil_stream(rng, i)
        got, st = J.decode_luma(b)
        assert st == J.OK, i
        assert np.array_equal(got, pil_luma(b)), i


@needs_pil
def test_pillow_decodes_numpy_streams_to_the_same_luma():
    rng = np.random.default_rng(7)
    for i in range(40):
        samp = ["444", "422", "440", "420", "grey"][i % 5]
        w, h = int(rng.integers(8, 60)), int(rng.integers(8, 60))
        luma = (rng.random((h, w)) * 255).astype(np.uint8) if i % 2 else (np.add.outer(np.arange(h), np.arange(w)) * 4 % 256).astype(np.uint8)
        kw = dict(sampling=samp, quality=[30, 85, 100, 5][i % 4], restart_interval=[0, 1, 7, 3][(i // 5) % 4], dht=i % 7 != 3,
                  q16=i % 6 == 5)
        if i % 8 == 6:
            kw["tables"] = {(0, 0): J.shuffled_table(0, 0, rng), (1, 0): J.shuffled_table(1, 0, rng), (1, 1): J.shuffled_table(1, 1, rng)}
            kw["dht"] = True
        b = J.encode(luma, **kw)
        got, st = J.decode_luma(b)
        assert st == J.OK, (i, kw)
        assert np.array_equal(got, pil_luma(b)), (i, kw)


def test_idct_range_limit_masks_like_libjpeg():
    """An extreme DC wraps through libjpeg's range-limit table instead of clamping: the index is masked to 10 bits."""
    q = np.ones(64, np.int64)
    out = []
    for dc in (0, 1000, 1023, 4000, -4000, 8100, -8200, 32767, -32768):
        c = np.zeros((1, 64), np.int64)
        c[0, 0] = dc
        out.append(int(J.idct_islow(c, q)[0, 0, 0]))
    # DC d gives x = (d + 4) >> 3 after the two descales; range_limit[x & 1023]
    want = []
    for dc in (0, 1000, 1023, 4000, -4000, 8100, -8200, 32767, -32768):
        x = ((dc << 2) + 16) >> 5
        j = x & 1023
        want.append(j + 128 if j < 128 else 255 if j < 512 else 0 if j < 896 else j - 896)
    assert out == want
    assert out[5] != 255 and out[6] != 0   # 8100 and -8200 would clamp to 255 / 0; libjpeg's table wraps them


@needs_pil
def test_extreme_dc_wraps_as_libjpeg_c_islow():
    """Streams whose DCs land far outside the sample range (q1: DC quantiser 255): libjpeg's C jpeg_idct_islow wraps them
    through its masked range-limit table, and the numpy restatement returns the same bytes.  libjpeg-turbo's SIMD IDCT keeps a
    16-bit workspace that overflows there instead (a different result), so libjpeg runs with its own JSIMD_FORCENONE=1 switch,
    in a child process."""
    import subprocess
    rng = np.random.default_rng(17)
    luma = (rng.random((32, 48)) * 255).astype(np.uint8)
    streams = [J.encode(luma, sampling="444", quality=1, dc_offset=off) for off in (40, -40, 150, -150, 2000, np.arange(-300, 300, 7))]
    child = ("import io, sys, numpy as np\nfrom PIL import Image\n"
             "for h in sys.stdin.read().split():\n"
             "    im = Image.open(io.BytesIO(bytes.fromhex(h))); im.draft('L', im.size)\n"
             "    print(np.asarray(im.convert('L')).tobytes().hex())\n")
    r = subprocess.run([sys.executable, "-c", child], input=" ".join(b.hex() for b in streams), capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, JSIMD_FORCENONE="1"))
    assert r.returncode == 0, r.stderr[-500:]
    outs = r.stdout.split()
    assert len(outs) == len(streams)
    for b, o in zip(streams, outs):
        got, st = J.decode_luma(b)
        assert st == J.OK
        assert got.tobytes().hex() == o
        assert 0 < got.mean() < 255   # neither clamped to black nor to white


@needs_pil
def test_info_agrees_with_the_numpy_parser_and_pillow(built):
    rng = np.random.default_rng(99)
    for i in range(120):
        b = pil_stream(rng, i)
        rc, info = lib_info(b)
        nrc, ninfo = np_info(b)
        assert rc == nrc == A.CK_OK, i
        assert info == ninfo, i
        im = Image.open(io.BytesIO(b))
        assert (info["width"], info["height"]) == im.size
        assert info["n_components"] == (1 if im.mode == "L" else 3)
        assert info["has_dht"] == (0 if i % 6 == 4 else 1)


def test_info_on_numpy_streams(built):
    rng = np.random.default_rng(3)
    for samp, hv in (("444", (1, 1)), ("422", (2, 1)), ("440", (1, 2)), ("420", (2, 2)), ("grey", (1, 1))):
        luma = (rng.random((21, 37)) * 255).astype(np.uint8)
        b = J.encode(luma, sampling=samp, restart_interval=5, dht=False)
        rc, info = lib_info(b)
        assert rc == A.CK_OK and info == np_info(b)[1]
        assert (info["width"], info["height"], info["h_samp"], info["v_samp"]) == (37, 21) + hv
        assert (info["restart_interval"], info["has_dht"], info["n_components"]) == (5, 0, 1 if samp == "grey" else 3)


def _segments(b):
    """[(marker, start, end)] of the header segments up to and including SOS."""
    out, i = [], 2
    while i + 4 <= len(b):
        m, L = b[i + 1], (b[i + 2] << 8) | b[i + 3]
        out.append((m, i, i + 2 + L))
        if m == 0xDA:
            break
        i += 2 + L
    return out


def _patch(b, marker, fn):
    """The stream with the body of the first `marker` segment replaced by fn(body)."""
    for m, s, e in _segments(b):
        if m == marker:
            body = bytearray(b[s + 4:e])
            nb = bytes(fn(body))
            return b[:s + 2] + (len(nb) + 2).to_bytes(2, "big") + nb + b[e:]
    raise AssertionError("no marker %x" % marker)


def _remark(b, old, new):
    for m, s, e in _segments(b):
        if m == old:
            return b[:s + 1] + bytes([new]) + b[s + 2:]
    raise AssertionError("no marker %x" % old)


def test_info_refuses_each_rule_with_its_code(built):
    """One stream per rule, each valid but for that rule (cf. test_create_refuses_bad_families)."""
    rng = np.random.default_rng(5)
    luma = (rng.random((24, 40)) * 255).astype(np.uint8)
    good = J.encode(luma, sampling="420")
    assert lib_info(good)[0] == A.CK_OK
    cases = {}
    if Image is not None:
        buf = io.BytesIO()
        Image.fromarray(np.stack([luma] * 3, -1)).save(buf, "JPEG", progressive=True)
        cases["progressive"] = (buf.getvalue(), A.CK_EUNSUPPORTED)
    cases["SOF9 (arithmetic)"] = (_remark(good, 0xC0, 0xC9), A.CK_EUNSUPPORTED)
    sof1_12 = _patch(_remark(good, 0xC0, 0xC1), 0xC1, lambda s: bytes([12]) + s[1:])
    cases["12-bit SOF1"] = (sof1_12, A.CK_EUNSUPPORTED)
    cases["8-bit SOF1 is accepted"] = (_remark(good, 0xC0, 0xC1), A.CK_OK)
    cases["non-interleaved scan"] = (_patch(good, 0xDA, lambda s: bytes([1]) + s[1:3] + s[-3:]), A.CK_EUNSUPPORTED)
    cases["sampling 3x1"] = (_patch(good, 0xC0, lambda s: s[:7] + bytes([0x31]) + s[8:]), A.CK_EUNSUPPORTED)
    cases["chroma 2x1"] = (_patch(good, 0xC0, lambda s: s[:10] + bytes([0x21]) + s[11:]), A.CK_EUNSUPPORTED)
    cases["Y missing from the scan"] = (_patch(good, 0xDA, lambda s: bytes([2]) + s[3:7] + s[-3:]), A.CK_EUNSUPPORTED)
    dqt = [x for x in _segments(good) if x[0] == 0xDB][0]
    cases["truncated header"] = (good[:dqt[1] + 30], A.CK_EINVAL)
    cases["size < 4"] = (good[:3], A.CK_EINVAL)
    cases["missing SOI"] = (good[2:], A.CK_EINVAL)
    cases["EOI before the scan"] = (good[:dqt[1]] + b"\xff\xd9", A.CK_EINVAL)
    # a DHT that assigns the all-ones code (libjpeg refuses the table: JERR_BAD_HUFF_TABLE)
    cases["all-ones Huffman code"] = (_patch(good, 0xC4, lambda s: bytes([0x00, 2]) + bytes(15) + bytes([0, 1])), A.CK_EINVAL)
    for name, (b, want) in cases.items():
        rc, _ = lib_info(b)
        assert rc == want, (name, rc)
        assert np_info(b)[0] == want, (name, "numpy parser")
    # a null pointer
    from chalkydri_amd.detector import _bind
    from chalkydri_amd._lib import lib
    import ctypes as C
    info = A.JpegInfo()
    assert _bind(lib()).ck_jpeg_info(None, 100, C.byref(info)) == A.CK_EINVAL
    assert _bind(lib()).ck_jpeg_info(C.c_char_p(good), len(good), None) == A.CK_EINVAL
