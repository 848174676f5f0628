"""Raw camera formats and orientation, host side (no GPU): the numpy restatement (tests/raw_format_ref.py) against Pillow and
np.rot90, ck_raw_layout (the library's host-only validation) against it, the new symbols and their ctypes mirror, and the
convert kernels' code-object metadata (no scratch, no spills).  DESIGN.md §4d."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raw_format_ref as R  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402

try:
    from PIL import Image
except Exception:  # pragma: no cover
    Image = None
needs_pil = pytest.mark.skipif(Image is None, reason="Pillow is not importable")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ck_raw_layout", "ck_upload_raw", "ck_upload_raw_device", "ck_raw_luma_batch", "ck_ingest_create_raw")


@needs_pil
def test_luma_is_pillows_convert_L_on_all_colours():
    """L(R,G,B) of the contract is Pillow's Image.convert("L") on every one of the 2^24 colours."""
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    want = np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
    got = R.L(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    assert int((want != got).sum()) == 0


def test_luma_weights_sum_to_one():
    assert 19595 + 38470 + 7471 == 65536
    assert R.L(255, 255, 255) == 255 and R.L(0, 0, 0) == 0
    g = np.arange(256)
    assert np.array_equal(R.L(g, g, g), g)      # a grey pixel keeps its value: RGB and the Y formats agree on grey scenes


def test_orient_is_rot90():
    rng = np.random.default_rng(1)
    for sh, sw in ((5, 7), (16, 16), (33, 18)):
        S = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        assert np.array_equal(R.orient(S, "none"), S)
        assert np.array_equal(R.orient(S, "clockwise"), np.rot90(S, -1))
        assert np.array_equal(R.orient(S, "rotate-180"), np.rot90(S, 2))
        assert np.array_equal(R.orient(S, "counterclockwise"), np.rot90(S, 1))
        for o in R.ORIENTATIONS:
            assert np.array_equal(R.orient(S, o), R.orient_vec(S, o))
            assert np.array_equal(R.orient_vec(R.source_of(S, o), o), S)


def test_vectorised_luma_equals_the_loops():
    rng = np.random.default_rng(2)
    for fourcc in R.FOURCCS:
        for sw, sh, extra in ((16, 16, 0), (19, 17, 5), (33, 18, 24)):
            img = rng.integers(0, 256, (sh, sw, 3) if R.is_colour(fourcc) else (sh, sw), dtype=np.uint8)
            stride = R.min_stride(fourcc, sw) + extra
            buf = R.pack(img, fourcc, stride, seed=sw)
            a, b = R.luma(buf, fourcc, sw, sh, stride), R.luma_vec(buf, fourcc, sw, sh, stride)
            assert np.array_equal(a, b), fourcc
            want = R.L(img[..., 0], img[..., 1], img[..., 2]) if R.is_colour(fourcc) else img
            assert np.array_equal(a, want), fourcc


def _layout(fourcc, w, h, o):
    from chalkydri_amd.detector import _bind, fourcc as cc
    from chalkydri_amd._lib import lib
    fmt = A.RawFormat(cc(fourcc), o)
    sw, sh, ms, mb = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
    rc = _bind(lib()).ck_raw_layout(C.byref(fmt), w, h, C.byref(sw), C.byref(sh), C.byref(ms), C.byref(mb))
    return rc, (sw.value, sh.value, ms.value, mb.value)


def test_raw_layout_every_format_and_orientation(built):
    assert set(A.RAW_FOURCCS) == set(R.FOURCCS)
    for fourcc in R.FOURCCS:
        for o, name in enumerate(R.ORIENTATIONS):
            assert A.ORIENTATIONS[name] == o
            for w, h in ((16, 16), (640, 480), (641, 479), (1280, 800), (17, 4095), (1, 1)):
                rc, got = _layout(fourcc, w, h, o)
                sw, sh = R.source_size(w, h, name)
                ms = R.min_stride(fourcc, sw)
                assert rc == A.CK_OK and got == (sw, sh, ms, sh * ms), (fourcc, name, w, h, got)
    # 4:2:2 rows hold whole pixel pairs; the colour formats are 3 and 4 bytes per pixel
    assert _layout("YUYV", 641, 479, 0)[1][2] == 1284 and _layout("UYVY", 479, 641, 1)[1][2] == 1284
    assert _layout("RGB ", 641, 479, 2)[1][2] == 1923 and _layout("BGRA", 641, 479, 3)[1][:3] == (479, 641, 1916)


def test_raw_layout_refusals(built):
    from chalkydri_amd.detector import _bind, fourcc as cc, raw_layout
    from chalkydri_amd._lib import ChalkydriError, lib
    L = _bind(lib())
    for bad in ("MJPG", "H264", "BA81", "Y16 ", "P010", "ARGB", "yuyv"):
        assert _layout(bad, 640, 480, 0)[0] == A.CK_EUNSUPPORTED, bad
    for o in (-1, 4, 90, 180):
        assert _layout("YUYV", 640, 480, o)[0] == A.CK_EINVAL
    assert _layout("YUYV", 0, 480, 0)[0] == A.CK_EINVAL and _layout("GREY", 640, -1, 0)[0] == A.CK_EINVAL
    fmt = A.RawFormat(cc("YUYV"), 0)
    a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    assert L.ck_raw_layout(None, 640, 480, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == A.CK_EINVAL
    assert L.ck_raw_layout(C.byref(fmt), 640, 480, None, C.byref(b), C.byref(c), C.byref(d)) == A.CK_EINVAL
    assert L.ck_raw_layout(C.byref(fmt), 640, 480, C.byref(a), None, C.byref(c), C.byref(d)) == A.CK_EINVAL
    assert L.ck_raw_layout(C.byref(fmt), 640, 480, C.byref(a), C.byref(b), None, C.byref(d)) == A.CK_EINVAL
    assert L.ck_raw_layout(C.byref(fmt), 640, 480, C.byref(a), C.byref(b), C.byref(c), None) == A.CK_EINVAL
    # the Python layer: the reference's serde names, and errors as exceptions
    assert raw_layout("YUYV", 480, 640, "counterclockwise") == (640, 480, 1280, 480 * 1280)
    with pytest.raises(ChalkydriError) as e:
        raw_layout("MJPG", 640, 480)
    assert e.value.code == A.CK_EUNSUPPORTED
    with pytest.raises(ValueError):
        raw_layout("YUYV", 640, 480, "upside-down")


def test_new_symbols_are_exported_declared_and_mirrored(built):
    from chalkydri_amd.detector import AprilTagDetector, IngestRing, _bind
    from chalkydri_amd._lib import lib
    L = _bind(lib())
    header = open(os.path.join(ROOT, "include", "chalkydri_hip.h")).read()
    for name in NEW_SYMBOLS:
        fn = getattr(L, name)                                   # AttributeError = not exported
        assert fn.argtypes is not None, name                    # bound with a prototype in detector._bind
        assert re.search(r"\bint %s\(" % name, header), name
    assert L.ck_abi_version() == 3                              # additions only
    m = re.search(r"typedef struct ck_raw_format \{\s*uint32_t fourcc;\s*int32_t orientation;\s*\} ck_raw_format_t;", header)
    assert m and C.sizeof(A.RawFormat) == 8 and [f[0] for f in A.RawFormat._fields_] == ["fourcc", "orientation"]
    for name, val in (("CK_ORIENT_NONE", 0), ("CK_ORIENT_CLOCKWISE", 1), ("CK_ORIENT_ROTATE_180", 2), ("CK_ORIENT_COUNTERCLOCKWISE", 3)):
        assert re.search(r"\b%s = %d\b" % (name, val), header) and getattr(A, name) == val
    for meth in ("upload_raw", "upload_raw_device", "raw_luma"):
        assert callable(getattr(AprilTagDetector, meth))
    assert "fourcc" in IngestRing.__init__.__code__.co_varnames and "orientation" in IngestRing.__init__.__code__.co_varnames


def test_convert_kernels_use_no_scratch(built):
    """The code object's own metadata (as test_abi.py reads it for the fit kernels): every instantiation of the two convert
    kernels — 4 pixel sizes x 4 orientations — is there, and none has scratch or a spilled register."""
    import shutil
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    obj = "k_rawfmt.o"
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
    kernels = {k: v for k, v in res.items() if "k_raw_straight" in k or "k_raw_quarter" in k}
    assert len(kernels) == 16, sorted(kernels)
    for k, v in kernels.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["vgpr_count"] <= 64, (k, v)    # 8 waves per SIMD: a streaming kernel lives on its occupancy
