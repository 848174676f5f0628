"""CPU: the restatements the colour preview's GPU tests compare against.  tests/np_jpeg_enc_color.py equals
libjpeg(-turbo) as Pillow drives it, byte for byte, whole files; libjpeg's colour conversion is the stated formulas for all 2^24
colours; the index arithmetic of tests/preview_color_ref.py in loops equals its vectorised form; ck_preview_color_layout without
a device; the new kernels' code objects."""
import ctypes as C
import io
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg_enc as E  # noqa: E402
import np_jpeg_enc_color as EC  # noqa: E402
import preview_color_ref as PC  # noqa: E402
import raw_format_ref as R  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 8), (9, 9), (17, 13), (40, 24), (640, 480)]
QUALITIES = [1, 25, 50, 85, 100]
RESTARTS = [0, 1, 3]
KINDS = ["flat", "ramp", "smooth", "noise"]


def pillow():
    return pytest.importorskip("PIL.Image")


def pillow_encode(P, mode, q, rr):
    buf = io.BytesIO()
    kw = {"restart_marker_rows": rr} if rr else {}
    pillow().fromarray(np.ascontiguousarray(P), mode).save(buf, "JPEG", quality=q, subsampling=0, optimize=False, **kw)
    return buf.getvalue()


def content(rng, kind, h, w):
    """(Y, Cb, Cr) images from flat to noise, the three planes unlike each other."""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "flat":
        return np.broadcast_to(np.array([97, 200, 31], np.uint8), (h, w, 3)).copy()
    if kind == "ramp":
        return np.stack([(xx * 3 + yy * 2) % 256, (xx * 5 + yy) % 256, (255 - xx * 2 + yy * 7) % 256], -1).astype(np.uint8)
    if kind == "smooth":
        f = [128 + 90 * np.sin(xx / a) * np.cos(yy / b) + rng.normal(0, 3, (h, w)) for a, b in ((9.0, 13.0), (5.0, 21.0), (17.0, 4.0))]
        return np.clip(np.stack(f, -1), 0, 255).astype(np.uint8)
    assert kind == "noise"
    return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)


@pytest.fixture(scope="module")
def longest():
    """Longest file of the Pillow comparison per (w, h, restart_rows): what the layout test bounds."""
    return {}


def test_whole_files_equal_pillow(longest):
    """encode_ycc is byte-equal to Pillow's save from mode YCbCr (4:4:4): 5 sizes (8 x 8, both dimensions != 0 mod 8, 640 x 480) x
    qualities 1, 25, 50, 85, 100 x restart_rows 0, 1, 3 x content flat to noise.  Noise at quality 100 fills all three components
    with FF bytes (asserted).  The loop form of the entropy coder is compared on the small sizes."""
    rng = np.random.default_rng(12)
    assert pillow_encode(np.zeros((32, 32, 3), np.uint8), "YCbCr", 50, 0) != pillow_encode(np.zeros((32, 32, 3), np.uint8), "YCbCr", 50, 1)
    cases, bad = 0, []
    for si, (w, h) in enumerate(SIZES):
        for qi, q in enumerate(QUALITIES):
            for rr in RESTARTS:
                # at 640 x 480 two kinds per cell, rotating so every kind meets every quality and restart value; all four below it
                kinds = KINDS if w < 640 else [KINDS[(qi + rr + k) % 4] for k in range(2)]
                if q == 100 and "noise" not in kinds:
                    kinds = kinds[:1] + ["noise"]
                for kind in kinds:
                    P = content(rng, kind, h, w)
                    got = EC.encode_ycc(P, q, rr)
                    cases += 1
                    longest[(w, h, rr)] = max(longest.get((w, h, rr), 0), len(got))
                    if got != pillow_encode(P, "YCbCr", q, rr):
                        bad.append((w, h, q, rr, kind))
                    if w <= 17 and EC.encode_ycc(P, q, rr, EC.entropy_items) != got:
                        bad.append((w, h, q, rr, kind, "loops"))
                    if kind == "noise" and q == 100 and w >= 40:
                        assert got.count(b"\xff\x00") > 3, (w, h, rr)
    print(f"{cases} cases")
    assert cases >= 250 and not bad, (len(bad), bad[:10])


def test_stuffing_in_every_component():
    """A noise image at quality 100 where only one component is noise still has stuffed FF bytes: each component makes them."""
    rng = np.random.default_rng(5)
    for c in range(3):
        P = np.full((64, 64, 3), 128, np.uint8)
        P[:, :, c] = rng.integers(0, 256, (64, 64))
        b = EC.encode_ycc(P, 100, 0)
        assert b == pillow_encode(P, "YCbCr", 100, 0) and b.count(b"\xff\x00") > 0, c


def test_every_colour_converts_as_libjpeg_does():
    """The 4096 x 4096 image of all 2^24 colours: Pillow's file from mode RGB (libjpeg's own rgb_ycc_convert) equals its file
    from mode YCbCr fed with the formulas of §4g.  Quality 100: the quantiser's smallest steps, so that a conversion off by one
    anywhere changes the file."""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    rgb = np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8)
    yc = EC.rgb_to_ycc(rgb)
    assert pillow_encode(rgb, "RGB", 100, 0) == pillow_encode(yc, "YCbCr", 100, 0)
    assert EC.OVERLAY_TRIPLE == (150, 44, 21)
    g = np.arange(256, dtype=np.uint8)
    assert np.array_equal(EC.ycc(g, g, g)[0], g) and np.all(EC.ycc(g, g, g)[1] == 128) and np.all(EC.ycc(g, g, g)[2] == 128)
    assert np.array_equal(yc[..., 0], R.L(rgb[..., 0], rgb[..., 1], rgb[..., 2]))       # Y is §4d's L: the staged luma


def test_rgb_file_equals_ycc_restatement():
    """End to end on the CPU: Pillow's save of an RGB picture equals encode_ycc of its converted triples."""
    rng = np.random.default_rng(9)
    for (w, h), q, rr in [((40, 24), 50, 0), ((17, 13), 85, 1), ((9, 9), 100, 3)]:
        rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        assert EC.encode_ycc(EC.rgb_to_ycc(rgb), q, rr) == pillow_encode(rgb, "RGB", q, rr), (w, h, q, rr)


def test_worst_block_fits_the_bound():
    """The 264-byte worst-case block of §4c / §4e holds for the chrominance tables as for the luminance ones."""
    bits = [EC.worst_block_bits(t) for t in range(2)]
    print("worst block bits (luminance, chrominance):", bits)
    assert bits == [1658, 1660] and max(bits) <= 8 * E.BLOCK_MAX_BYTES
    # no item is longer than the bit writer's 27-bit step
    for dc, ac in EC.TABLES:
        assert max(int(dc[s, 1]) + s for s in range(12)) <= 27 and max(int(ac[(r << 4) | s, 1]) + s for r in range(16) for s in range(1, 11)) <= 27


def test_index_arithmetic_loops_equal_the_vectorised_form():
    """Steps 1-3 as loops equal the vectorised form: every family x orientation, odd source widths (the half-filled last pair of
    the 4:2:2 formats), strides above the minimum, identity and non-integer scales, with and without an overlay."""
    rng = np.random.default_rng(21)
    quad = [np.array([[3.5, 2.25], [20.0, 4.0], [22.75, 15.5], [2.0, 17.0]])]
    for fourcc in PC.FAMILIES:
        for oi, o in enumerate(R.ORIENTATIONS):
            for (W, H), (pw, ph) in [((27, 19), (27, 19)), ((27, 19), (13, 9)), ((30, 21), (8, 8))]:
                sw, sh = R.source_size(W, H, o)
                stride = R.min_stride(fourcc, sw) + (5 if oi % 2 else 0)
                buf = PC.pack_colour(rng, fourcc, sw, sh, stride)
                for dets in (None, quad):
                    a = PC.triples(buf, fourcc, sw, sh, stride, o, pw, ph, dets)
                    b = PC.triples_vec(buf, fourcc, sw, sh, stride, o, pw, ph, dets)
                    assert np.array_equal(a, b), (fourcc, o, W, H, pw, ph, dets is not None)
                    if dets is not None:
                        assert (a == np.array(EC.OVERLAY_TRIPLE, np.uint8)).all(-1).any()
    # the luma plane of the triples is what §4d stages
    buf = PC.pack_colour(rng, "UYVY", 27, 19)
    assert np.array_equal(PC.triples_vec(buf, "UYVY", 27, 19, 56, "clockwise", 19, 27)[..., 0], R.expected(buf, "UYVY", 27, 19, 56, "clockwise"))


def test_color_layout(built, longest):
    """ck_preview_color_layout: ck_preview_layout's sizes and refusals, the colour file's bound — value for value the
    restatement's, and never below the longest file of the Pillow comparison."""
    from chalkydri_amd.detector import preview_color_layout, preview_layout, preview_params, _bind
    from chalkydri_amd._lib import ChalkydriError, lib
    L = _bind(lib())
    pp = preview_params()
    assert L.ck_preview_color_layout(C.byref(pp), 640, 480, None, None, None) == A.CK_OK
    assert L.ck_preview_color_layout(None, 640, 480, None, None, None) == A.CK_EINVAL

    def refused(W=640, H=480, **kw):
        try:
            preview_color_layout(preview_params(**kw), W, H)
        except ChalkydriError as e:
            return e.code == A.CK_EINVAL
        return False
    for kw in ({"width": 7}, {"height": 7}, {"width": -1}, {"height": -1}, {"quality": 0}, {"quality": 101}, {"restart_rows": -1},
               {"restart_rows": 820}, {"W": 0}, {"H": 0}, {"W": 7}, {"H": 5, "height": 0}):
        assert refused(**kw), kw
    assert not refused(restart_rows=819)                                       # DRI = 819 * 80 = 65520 MCUs
    for W, H, w, h, q, rr in [(1280, 800, 640, 480, 50, 0), (272, 200, 640, 480, 1, 3), (641, 479, 0, 0, 100, 1), (16, 16, 8, 8, 50, 7)]:
        got = preview_color_layout(preview_params(w, h, q, rr), W, H)
        assert got == EC.layout(w, h, W, H, q, rr)
        assert got[:2] == preview_layout(preview_params(w, h, q, rr), W, H)[:2]
    if not longest:
        test_whole_files_equal_pillow(longest)
    for (w, h, rr), n in longest.items():
        assert n <= preview_color_layout(preview_params(w, h, 100, rr), w, h)[2], (w, h, rr, n)
    assert len(EC.header(640, 480, 50, 0)) == EC.header_len(0) == 623 and len(EC.header(640, 480, 50, 80)) == EC.header_len(1) == 629


def test_new_symbols_are_exported_declared_and_mirrored(built):
    from chalkydri_amd.apriltags import AprilTags
    from chalkydri_amd.detector import AprilTagDetector, IngestRing, _bind
    from chalkydri_amd._lib import lib
    L = _bind(lib())
    header = open(os.path.join(ROOT, "include", "chalkydri_hip.h")).read()
    for name in ("ck_preview_color_layout", "ck_preview_jpeg_color", "ck_preview_jpeg_color_device", "ck_preview_jpeg_color_ingested",
                 "ck_preview_color", "ck_preview_color_device", "ck_preview_color_ingested"):
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert L.ck_abi_version() == 3                              # additions only
    for meth in ("preview_jpeg_color", "preview_color", "preview_jpeg_color_device", "preview_color_device"):
        assert callable(getattr(AprilTagDetector, meth))
    assert callable(IngestRing.preview_jpeg_color) and callable(IngestRing.preview_color)
    assert "color" in AprilTags.preview.__code__.co_varnames and AprilTags.preview.__defaults__[-1] is False


def test_colour_kernels_use_no_scratch(built):
    """The code object's own metadata: both instantiations of the colour front end and of the triples kernel, and the scan and
    pack kernels in both forms, are there; none has scratch or a spilled register — nor has the grey front end beside them."""
    import shutil
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    obj = "k_jpegenc.o"
    res, name = {}, None
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(os.path.join(ROOT, "chalkydri_amd", "csrc", "build", obj), td)
        subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", obj], cwd=td, stdout=subprocess.DEVNULL)
        co = [f for f in os.listdir(td) if f.startswith(obj) and "amdgcn" in f][0]
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], cwd=td, text=True)
        for line in notes.splitlines():
            m = re.match(r"\s*\.name:\s+(\S+)", line)
            if m:
                name = m.group(1)
                res[name] = {}
            m = re.match(r"\s*\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)", line)
            if m and name:
                res[name][m.group(1)] = int(m.group(2))
    count = lambda frag: len([k for k in res if frag in k])
    assert count("k_pv_fdct_color") == 2 and count("k_pv_color") == 2 and count("k_pv_scan") == 2 and count("k_pv_pack") == 2
    assert count("k_pv_fdct") == 3
    print({k: v["vgpr_count"] for k, v in res.items() if "k_pv_" in k})
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
