"""CPU: the planar 4:2:0 raw formats with their chroma planes, everything that needs no device.  ck_raw_layout and
ck_raw_plane_layout with CK_RAW_PLANES against the contract's formulas; every refusal in its order; ck_raw_ycc_host (the library's
one-thread twin of the colour triples) against tests/raw_planes_ref.py for the planar formats, against the restatements the colour
preview's tests already use for the packed ones, and of a planar frame against its YUYV twin; the loops of raw_planes_ref.py against
their vectorised form; the Python layer; the new symbols; the new kernels' code objects; ck_raw_planes.h under the sanitizers."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_color_ref as PC  # noqa: E402
import raw_format_ref as R  # noqa: E402
import raw_planes_ref as P  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 16), (17, 19), (34, 18), (641, 479), (17, 4095), (1, 1), (2, 2)]
EXTRA = (0, 2, 16)
FLAG = 0x100


def _L():
    from chalkydri_amd.detector import _bind
    from chalkydri_amd._lib import lib
    return _bind(lib())


def _fmt(code, o):
    from chalkydri_amd.detector import fourcc
    return A.RawFormat(fourcc(code), o)


def _layout(code, w, h, o):
    fmt = _fmt(code, o)
    sw, sh, ms, mb = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
    rc = _L().ck_raw_layout(C.byref(fmt), w, h, C.byref(sw), C.byref(sh), C.byref(ms), C.byref(mb))
    return rc, (sw.value, sh.value, ms.value, mb.value)


def _planes(code, w, h, o, stride):
    fmt, out = _fmt(code, o), A.RawPlanes()
    rc = _L().ck_raw_plane_layout(C.byref(fmt), w, h, stride, C.byref(out))
    return rc, out


def test_the_flag_collides_with_no_orientation_the_existing_tests_pass():
    assert A.CK_RAW_PLANES == FLAG == P.CK_RAW_PLANES
    for o in (-1, 4, 90, 180):
        assert o & ~(3 | FLAG), o       # each has a bit outside 0x103: still CK_EINVAL
    header = open(os.path.join(ROOT, "include", "chalkydri_hip.h")).read()
    assert re.search(r"#define CK_RAW_PLANES 0x100\b", header)


def test_layouts_against_the_formulas(built):
    for code in P.FOURCCS:
        for o, name in enumerate(R.ORIENTATIONS):
            for w, h in SHAPES:
                sw, sh = R.source_size(w, h, name)
                cw, ch = P.chroma_size(sw, sh)
                ms = 2 * cw
                rc, got = _layout(code, w, h, o | FLAG)
                assert rc == A.CK_OK and got == (sw, sh, ms, (sh + ch) * ms), (code, name, w, h, got)
                assert _layout(code, w, h, o) == (A.CK_OK, (sw, sh, sw, sh * sw))       # without the flag: as before
                for e in EXTRA:
                    stride = ms + e
                    rc, pl = _planes(code, w, h, o | FLAG, stride)
                    assert rc == A.CK_OK, (code, name, w, h, stride)
                    off, rs, st, total = P.formulas(code, sw, sh, stride)
                    assert (pl.sw, pl.sh, pl.cw, pl.ch) == (sw, sh, cw, ch)
                    assert tuple(pl.offset) == off and tuple(pl.row_stride) == rs and tuple(pl.step) == st and pl.bytes == total
                    assert tuple(pl.pad) == (0, 0)


def test_the_two_worked_examples(built):
    rc, pl = _planes("I420", 17, 19, A.CK_ORIENT_CLOCKWISE | FLAG, 24)
    assert rc == A.CK_OK and (pl.sw, pl.sh, pl.cw, pl.ch) == (19, 17, 10, 9)
    assert tuple(pl.offset) == (0, 408, 516) and tuple(pl.row_stride) == (24, 12, 12) and tuple(pl.step) == (1, 1, 1) and pl.bytes == 624
    rc, pl = _planes("NV21", 17, 19, A.CK_ORIENT_CLOCKWISE | FLAG, 24)
    assert rc == A.CK_OK and tuple(pl.offset) == (0, 409, 408) and tuple(pl.row_stride) == (24, 24, 24) and tuple(pl.step) == (1, 2, 2)
    assert pl.bytes == 624


def test_refusals_in_the_contracts_order(built):
    L = _L()
    out = A.RawPlanes()
    a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    # 1. a null fmt or a size below 1: CK_EINVAL, even with an unknown fourcc
    assert L.ck_raw_plane_layout(None, 16, 16, 16, C.byref(out)) == A.CK_EINVAL
    assert L.ck_raw_layout(None, 16, 16, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == A.CK_EINVAL
    assert _layout("H264", 0, 16, FLAG)[0] == A.CK_EINVAL and _planes("H264", 16, 0, FLAG, 16)[0] == A.CK_EINVAL
    # 2. an unknown fourcc: CK_EUNSUPPORTED, even with a bad orientation
    for bad in ("MJPG", "BA81", "Y16 ", "P010", "nv12"):
        assert _layout(bad, 16, 16, FLAG)[0] == A.CK_EUNSUPPORTED and _layout(bad, 16, 16, 4 | FLAG)[0] == A.CK_EUNSUPPORTED, bad
        assert _planes(bad, 16, 16, 0x200, 16)[0] == A.CK_EUNSUPPORTED
    # 3. any bit other than 0x103: CK_EINVAL, even where the flag could not apply
    for o in (-1, 4, 90, 180, 4 | FLAG, 0x200, 0x200 | FLAG, FLAG << 8, -FLAG):
        for code in ("NV12", "YV12", "GREY", "YUYV"):
            assert _layout(code, 16, 16, o)[0] == A.CK_EINVAL, (code, o)
            assert _planes(code, 16, 16, o, 16)[0] == A.CK_EINVAL, (code, o)
    # 4. the flag with a fourcc that has no chroma planes: CK_EUNSUPPORTED
    for code in ("GREY", "GRAY", "Y800", "YUYV", "YUY2", "UYVY", "RGB3", "RGB ", "BGR3", "BGR ", "RGBA", "BGRA"):
        for o in range(4):
            assert _layout(code, 16, 16, o | FLAG)[0] == A.CK_EUNSUPPORTED, code
            assert _planes(code, 16, 16, o | FLAG, 64)[0] == A.CK_EUNSUPPORTED, code
    # ck_raw_plane_layout alone: no flag, a null out, the stride
    for code in P.FOURCCS:
        assert _planes(code, 16, 16, 0, 16)[0] == A.CK_EUNSUPPORTED
        fmt = _fmt(code, FLAG)
        assert L.ck_raw_plane_layout(C.byref(fmt), 16, 16, 16, None) == A.CK_EINVAL
        assert _planes(code, 17, 19, FLAG, 17)[0] == A.CK_EINVAL          # sw for an odd sw is one byte short of 2 cw
        assert _planes(code, 17, 19, FLAG, 18)[0] == A.CK_OK
        assert _planes(code, 17, 19, FLAG, 19)[0] == (A.CK_EINVAL if code in ("I420", "YV12") else A.CK_OK)   # two half-stride planes
        assert _planes(code, 16, 16, FLAG, 15)[0] == A.CK_EINVAL and _planes(code, 16, 16, FLAG, 0)[0] == A.CK_EINVAL
    assert set(A.RAW_FOURCCS) == set(R.FOURCCS)                            # the table keeps its set


def _ycc(code, o, planes, frames, W, H):
    from chalkydri_amd.detector import raw_ycc_host
    return raw_ycc_host(frames, code, W, H, o, planes=planes)


def test_ycc_host_planar_equals_the_restatement_and_the_yuyv_twin(built):
    rng = np.random.default_rng(11)
    for code in P.FOURCCS:
        for o, name in enumerate(R.ORIENTATIONS):
            for w, h in [s for s in SHAPES if s[0] * s[1] <= 641 * 479]:
                sw, sh = R.source_size(w, h, name)
                for e in EXTRA if w * h < 10000 else (2,):
                    stride = P.min_stride(sw) + e
                    frames = [P.pack_planes(*P.random_planes(rng, sw, sh), code, stride, pad_byte=None, seed=k) for k in range(2)]
                    got = _ycc(code, name, True, frames, w, h)
                    assert got.shape == (2, h, w, 3)
                    for k in range(2):
                        want = P.triples_vec(frames[k], code, sw, sh, stride, name)
                        assert np.array_equal(got[k], want), (code, name, w, h, stride)
                    twins = [P.yuyv_twin(f, code, sw, sh, stride) for f in frames]
                    assert np.array_equal(_ycc("YUYV", name, False, twins, w, h), got), (code, name, w, h, stride)


def test_ycc_host_tall_frame(built):
    rng = np.random.default_rng(12)
    w, h = 17, 4095
    for code, name in (("NV12", "none"), ("YV12", "clockwise"), ("I420", "rotate-180"), ("NV21", "counterclockwise")):
        sw, sh = R.source_size(w, h, name)
        f = P.pack_planes(*P.random_planes(rng, sw, sh), code, P.min_stride(sw) + 2, pad_byte=None, seed=3)
        assert np.array_equal(_ycc(code, name, True, [f], w, h)[0], P.triples_vec(f, code, sw, sh, P.min_stride(sw) + 2, name))


def test_ycc_host_packed_equals_the_existing_restatements(built):
    """The packed families through the restatement the colour preview's tests compare the kernels with (preview_color_ref.py on
    raw_format_ref.py's formats and np_jpeg_enc_color.py's conversion)."""
    rng = np.random.default_rng(13)
    for code in PC.FAMILIES + ("YUY2", "RGB ", "BGR "):
        for o, name in enumerate(R.ORIENTATIONS):
            for w, h in ((16, 16), (17, 19), (34, 18), (1, 1)):
                sw, sh = R.source_size(w, h, name)
                for e in (0, 5):
                    stride = R.min_stride(code, sw) + e
                    f = PC.pack_colour(rng, code, sw, sh, stride)
                    want = PC.triples_vec(f, code, sw, sh, stride, name, w, h)
                    assert np.array_equal(_ycc(code, name, False, [f], w, h)[0], want), (code, name, w, h, stride)


def test_ycc_host_refusals(built):
    from chalkydri_amd._lib import ChalkydriError
    f = np.zeros((24, 16), np.uint8)
    for code in R.LUMA_FIRST:                      # a luma-first fourcc without the flag has no colour
        with pytest.raises(ChalkydriError) as e:
            _ycc(code, "none", False, [f], 16, 16)
        assert e.value.code == A.CK_EUNSUPPORTED
    with pytest.raises(ChalkydriError) as e:
        _ycc("GREY", "none", True, [f], 16, 16)
    assert e.value.code == A.CK_EUNSUPPORTED
    L = _L()
    fmt = _fmt("I420", FLAG)
    img = (A.ImageU8 * 1)()
    img[0].buf, img[0].width, img[0].height, img[0].stride = f.ctypes.data, 16, 16, 16
    out = np.zeros((16, 16, 3), np.uint8)
    assert L.ck_raw_ycc_host(C.byref(fmt), img, 1, 16, 16, out.ctypes.data) == A.CK_OK
    assert L.ck_raw_ycc_host(C.byref(fmt), img, 1, 16, 16, None) == A.CK_EINVAL
    assert L.ck_raw_ycc_host(C.byref(fmt), None, 1, 16, 16, out.ctypes.data) == A.CK_EINVAL
    assert L.ck_raw_ycc_host(C.byref(fmt), img, -1, 16, 16, out.ctypes.data) == A.CK_EINVAL
    img[0].width = 15
    assert L.ck_raw_ycc_host(C.byref(fmt), img, 1, 16, 16, out.ctypes.data) == A.CK_EINVAL
    img[0].width, img[0].stride = 16, 17           # odd, with two half-stride planes
    assert L.ck_raw_ycc_host(C.byref(fmt), img, 1, 16, 16, out.ctypes.data) == A.CK_EINVAL
    img[0].stride = 14
    assert L.ck_raw_ycc_host(C.byref(fmt), img, 1, 16, 16, out.ctypes.data) == A.CK_EINVAL


def test_loops_equal_the_vectorised_form():
    rng = np.random.default_rng(14)
    for code in P.FOURCCS:
        for o, name in enumerate(R.ORIENTATIONS):
            for w, h in ((16, 16), (17, 19), (34, 18), (1, 1), (2, 2)):
                sw, sh = R.source_size(w, h, name)
                for e in EXTRA:
                    stride = P.min_stride(sw) + e
                    y, cb, cr = P.random_planes(rng, sw, sh)
                    f = P.pack_planes(y, cb, cr, code, stride)
                    a = P.triples(f, code, sw, sh, stride, name)
                    assert np.array_equal(a, P.triples_vec(f, code, sw, sh, stride, o)), (code, name, w, h, stride)
                    # ... and both are the three arrays, chroma replicated, turned as raw_format_ref.py turns luma
                    S = np.stack([y, np.repeat(np.repeat(cb, 2, 0), 2, 1)[:sh, :sw], np.repeat(np.repeat(cr, 2, 0), 2, 1)[:sh, :sw]], -1)
                    for c in range(3):
                        assert np.array_equal(a[..., c], R.orient_vec(S[..., c], name))
                    # the padding is never part of a triple
                    g = P.pack_planes(y, cb, cr, code, stride, pad_byte=None, seed=5)
                    assert np.array_equal(P.triples_vec(g, code, sw, sh, stride, o), a)
                    # the twin is a YUYV frame with the same triples, by the restatement that was there before
                    t = P.yuyv_twin(f, code, sw, sh, stride)
                    assert t.shape == (sh, R.min_stride("YUYV", sw))
                    assert np.array_equal(PC.triples_vec(t, "YUYV", sw, sh, t.shape[1], name, w, h), a)


def test_python_layer(built):
    from chalkydri_amd import detector as D
    from chalkydri_amd._lib import ChalkydriError
    assert D.raw_format("NV12", "clockwise", planes=True).orientation == 1 | FLAG
    assert D.raw_format("NV12", "clockwise").orientation == 1 and D.raw_format("NV12", 1 | FLAG).orientation == 1 | FLAG
    assert D.raw_layout("NV12", 17, 19, "clockwise", planes=True) == (19, 17, 20, 26 * 20)
    assert D.raw_layout("NV12", 17, 19, "clockwise") == (19, 17, 19, 17 * 19)
    pl = D.raw_plane_layout("I420", 17, 19, 24, "clockwise")
    assert pl == {"sw": 19, "sh": 17, "cw": 10, "ch": 9, "offset": (0, 408, 516), "row_stride": (24, 12, 12), "step": (1, 1, 1), "bytes": 624}
    with pytest.raises(ChalkydriError) as e:
        D.raw_layout("YUYV", 16, 16, planes=True)
    assert e.value.code == A.CK_EUNSUPPORTED
    with pytest.raises(ChalkydriError) as e:
        D.raw_plane_layout("NV12", 17, 19, 17)
    assert e.value.code == A.CK_EINVAL
    with pytest.raises(ValueError):
        D.raw_ycc_host([np.zeros((16, 16), np.uint8)], "NV12", 16, 16, planes=True)    # 24 rows with the planes
    for meth in ("upload_raw", "raw_luma", "upload_raw_device", "preview_jpeg_color_device", "preview_color_device", "detect_blobs_device",
                 "blob_time"):
        assert "planes" in getattr(D.AprilTagDetector, meth).__code__.co_varnames, meth
    assert "planes" in D.IngestRing.__init__.__code__.co_varnames
    from chalkydri_amd.apriltags import AprilTags
    assert "planes" in AprilTags.__init__.__code__.co_varnames
    assert A.PLANAR_FOURCCS == P.FOURCCS


def test_new_symbols_are_exported_declared_and_mirrored(built):
    L = _L()
    header = open(os.path.join(ROOT, "include", "chalkydri_hip.h")).read()
    for name in ("ck_raw_plane_layout", "ck_raw_ycc_host"):
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert L.ck_abi_version() == 3                              # additions only
    assert C.sizeof(A.RawPlanes) == 80 and A.RawPlanes.offset.offset == 16 and A.RawPlanes.row_stride.offset == 40
    assert A.RawPlanes.step.offset == 52 and A.RawPlanes.bytes.offset == 72 and C.sizeof(A.RawFormat) == 8
    m = re.search(r"typedef struct ck_raw_planes \{(.*?)\} ck_raw_planes_t;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d\])?\s*[,;]", body) == [f[0] for f in A.RawPlanes._fields_]
    rust = open(os.path.join(ROOT, "rust", "chalkydri_hip_sys", "src", "lib.rs")).read()
    assert "pub const CK_RAW_PLANES: i32 = 0x100;" in rust and "pub struct ck_raw_planes_t" in rust
    assert "pub fn ck_raw_plane_layout(" in rust and "pub fn ck_raw_ycc_host(" in rust
    hpp = open(os.path.join(ROOT, "include", "chalkydri.hpp")).read()
    assert "bool planes = false" in hpp and "raw_plane_layout(" in hpp and "bool raw_planes = false;" in hpp


def _notes(obj):
    import shutil
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
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
        m = re.match(r"\s*\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_count):\s+(\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    return res


def test_planar_kernels_use_no_scratch_and_no_lds_of_their_own(built):
    """One kernel per consumer for the new source kind, from the code objects' own metadata: no private segment, no spill; the
    triples and the two blob kernels hold no LDS at all, the front end only the encoder tables its 4:2:2 sibling holds."""
    pv, bl = _notes("k_jpegenc.o"), _notes("k_blobs.o")
    one = lambda res, frag: [v for k, v in res.items() if frag in k]
    for res, frag in ((pv, "k_pv_ptriples"), (pv, "k_pv_pfdct"), (bl, "k_blob_prgb"), (bl, "k_blob_pmask")):
        got = one(res, frag)
        assert len(got) == 1, frag
        v = got[0]
        print(frag, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (frag, v)
    for res, frag in ((pv, "k_pv_ptriples"), (bl, "k_blob_prgb"), (bl, "k_blob_pmask")):
        assert one(res, frag)[0]["group_segment_fixed_size"] == 0, frag
    sib = [v for k, v in pv.items() if "k_pv_fdct_color" in k]
    assert one(pv, "k_pv_pfdct")[0]["group_segment_fixed_size"] == sib[0]["group_segment_fixed_size"]


def test_plane_map_under_sanitizers(built):
    """csrc/ck_raw_planes.h alone under AddressSanitizer + UBSan, driven by tests/cpp/raw_planes_check.cpp: exact-size buffers."""
    check = os.path.join(ROOT, "chalkydri_amd", "lib", "raw_planes_check")
    r = subprocess.run([check], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "raw_planes_check ok" in r.stdout
