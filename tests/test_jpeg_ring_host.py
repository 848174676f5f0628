"""MJPEG through the ingest ring, turned by the camera's mounting: the host side (no GPU).  The five new entry points are exported,
declared and mirrored (ctypes, Rust), the ABI version stays 3, and the argument checks that need no device answer as the header
says.  DESIGN.md §4c, "JPEG frames: orientation and the ring"."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg as J  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ck_upload_jpeg_oriented", "ck_jpeg_luma_batch_oriented", "ck_ingest_create_jpeg", "ck_ingest_write_jpeg",
               "ck_ingest_jpeg_status")


def _L():
    from chalkydri_amd.detector import _bind
    from chalkydri_amd._lib import lib
    return _bind(lib())


def test_new_symbols_are_exported_declared_and_mirrored(built):
    L = _L()
    header = open(os.path.join(ROOT, "include", "chalkydri_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "chalkydri_hip_sys", "src", "lib.rs")).read()
    for name in NEW_SYMBOLS:
        fn = getattr(L, name)                                   # AttributeError = not exported
        assert fn.argtypes is not None, name                    # bound with a prototype in detector._bind
        assert re.search(r"\bint %s\(" % name, header), name
        assert len(re.findall(r"pub fn %s\(" % name, rust)) == 1, name
    assert L.ck_abi_version() == 3                              # additions only
    assert re.search(r"#define CK_ABI_VERSION 3\b", header)


def test_oriented_upload_refuses_before_touching_a_device(built):
    """A null handle, null frames, n < 0 and an orientation outside 0..3 are CK_EINVAL; a handle cannot exist without a device, so
    the checks that need one stand in for it with a pointer the library must not follow."""
    from chalkydri_amd.detector import _jpeg_frames
    L = _L()
    b = J.encode(np.full((16, 16), 99, np.uint8))
    arr, keep = _jpeg_frames([b])
    st = (C.c_uint32 * 1)()
    out = np.zeros((16, 16), np.uint8)
    assert L.ck_upload_jpeg_oriented(None, arr, 1, 0, st) == A.CK_EINVAL
    assert L.ck_jpeg_luma_batch_oriented(None, arr, 1, 0, out.ctypes.data, st) == A.CK_EINVAL
    fake = C.c_void_p(8)   # not a handle: every refusal below must come before the first read through it
    assert L.ck_upload_jpeg_oriented(fake, None, 1, 0, st) == A.CK_EINVAL
    assert L.ck_upload_jpeg_oriented(fake, arr, -1, 0, st) == A.CK_EINVAL
    assert L.ck_upload_jpeg_oriented(fake, arr, 1, 4, st) == A.CK_EINVAL
    assert L.ck_upload_jpeg_oriented(fake, arr, 1, -1, st) == A.CK_EINVAL
    assert L.ck_jpeg_luma_batch_oriented(fake, arr, 1, 0, None, st) == A.CK_EINVAL
    assert L.ck_jpeg_luma_batch_oriented(fake, arr, 1, 7, out.ctypes.data, st) == A.CK_EINVAL


def test_ring_entry_points_refuse_null_arguments(built):
    L = _L()
    g = C.c_void_p()
    fake = C.c_void_p(8)
    assert L.ck_ingest_create_jpeg(None, 2, 0, 0, C.byref(g)) == A.CK_EINVAL
    assert L.ck_ingest_create_jpeg(fake, 2, 4, 0, C.byref(g)) == A.CK_EINVAL
    assert L.ck_ingest_create_jpeg(fake, 2, -1, 0, C.byref(g)) == A.CK_EINVAL
    assert L.ck_ingest_create_jpeg(fake, 2, 0, -1, C.byref(g)) == A.CK_EINVAL
    assert L.ck_ingest_create_jpeg(fake, 0, 0, 0, C.byref(g)) == A.CK_EINVAL
    assert L.ck_ingest_create_jpeg(fake, 9, 0, 0, C.byref(g)) == A.CK_EINVAL
    assert L.ck_ingest_create_jpeg(fake, 2, 0, 0, None) == A.CK_EINVAL
    data = np.zeros(16, np.uint8)
    st = (C.c_uint32 * 1)()
    assert L.ck_ingest_write_jpeg(None, 0, 0, data.ctypes.data, 16) == A.CK_EINVAL
    assert L.ck_ingest_jpeg_status(None, 0, 0, st) == A.CK_EINVAL


def test_python_ring_refuses_an_unknown_fourcc_name(built):
    """The name is resolved on the host: neither "H264" nor a lower-case "mjpg" reaches the device layer."""
    from chalkydri_amd._lib import ChalkydriError
    from chalkydri_amd.detector import IngestRing

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the ring called %s before refusing the fourcc" % name)
    det = types.SimpleNamespace(_L=NoDevice(), _h=None, width=640, height=480, cfg=types.SimpleNamespace(height=480, max_batch=1))
    for bad in ("H264", "mjpg", "BA81"):
        with pytest.raises(ChalkydriError) as e:
            IngestRing(det, 2, fourcc=bad)
        assert e.value.code == A.CK_EUNSUPPORTED, bad
    with pytest.raises(ValueError):
        IngestRing(det, 2, fourcc="MJPG", orientation="upside-down")
    assert A.JPEG_FOURCCS == ("MJPG", "JPEG") and not set(A.JPEG_FOURCCS) & set(A.RAW_FOURCCS)
    assert {"fourcc", "orientation", "max_frame_bytes"} <= set(IngestRing.__init__.__code__.co_varnames)
    assert callable(IngestRing.jpeg_status)


def test_apriltags_takes_mjpg_up_to_the_device(built):
    """AprilTags(fourcc="MJPG") gets as far as the raw-format constructor does: to ck_create, which needs a device."""
    import scenes
    from chalkydri_amd._lib import ChalkydriError
    from chalkydri_amd.apriltags import AprilTags
    from chalkydri_amd.detector import AprilTagDetector, device_count
    layout = scenes.wall_layout(2, cols=2)
    calib = {"OpenCVModel5": dict(fx=600.0, fy=600.0, cx=240.0, cy=320.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)}
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.0, "y": 0.0, "z": 0.0}
    with pytest.raises(ValueError):
        AprilTags(480, 640, layout, calib, r2c, fourcc="MJPG", orientation="sideways")
    outcomes = []
    for fourcc in ("YUYV", "MJPG"):
        try:
            task = AprilTags(480, 640, layout, calib, r2c, fourcc=fourcc, orientation="clockwise")
            outcomes.append("built")
            assert task.fourcc == fourcc and callable(task.process_raw)
            task.detector.close()
        except ChalkydriError as e:
            outcomes.append(e.code)
    assert outcomes[0] == outcomes[1]
    assert outcomes[0] == ("built" if device_count() > 0 else A.CK_ENODEVICE)
    assert "orientation" in AprilTagDetector.upload_jpeg.__code__.co_varnames
    assert "orientation" in AprilTagDetector.decode_jpeg.__code__.co_varnames


def test_cpp_header_and_demo_declare_the_mjpeg_surface(built):
    src = open(os.path.join(ROOT, "include", "chalkydri.hpp")).read()
    for name in ("upload_jpeg(const std::vector<std::vector<uint8_t>> &jpegs, int32_t orientation", "ck_ingest_create_jpeg", "write_jpeg(",
                 "jpeg_status(", "process_jpeg(", "is_jpeg_fourcc("):
        assert name in src, name
    assert os.path.exists(os.path.join(ROOT, "chalkydri_amd", "lib", "jpeg_ring_demo"))
