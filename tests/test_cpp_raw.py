"""The raw-format entry points of the C++ host layer (include/chalkydri.hpp: raw_format, raw_layout, Handle::upload_raw /
raw_luma, AprilTags::Config::{fourcc, orientation}) through tests/cpp/raw_demo.cpp: the layout without a GPU, and on a GPU the
staged luma byte-equal to the numpy restatement and the detector finding the scene's tags behind it."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raw_format_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "raw_demo")


def _run(*args):
    return subprocess.run([DEMO, *map(str, args)], capture_output=True, text=True, timeout=600)


def test_raw_demo_layout_needs_no_gpu(built):
    assert os.path.exists(DEMO)
    for fourcc, o, w, h in (("YUYV", "clockwise", 641, 479), ("RGB3", "none", 640, 480), ("BGRA", "rotate-180", 17, 33),
                            ("NV12", "counterclockwise", 1280, 800), ("RGB ", "none", 19, 16)):
        r = _run("layout", fourcc, o, w, h)
        sw, sh = R.source_size(w, h, o)
        ms = R.min_stride(fourcc, sw)
        assert r.returncode == 0 and r.stdout.split() == [str(sw), str(sh), str(ms), str(sh * ms)], (fourcc, o, r.stdout, r.stderr)
    assert _run("layout", "MJPG", "none", 640, 480).returncode == 3          # a Panic, as every refused call of the layer
    assert _run("layout", "YUYV", "upside-down", 640, 480).returncode == 3


def test_header_declares_the_raw_surface():
    src = open(os.path.join(ROOT, "include", "chalkydri.hpp")).read()
    for name in ("void upload_raw(", "void upload_raw_device(", "raw_luma(", "inline ck_raw_format_t raw_format(", "raw_layout(",
                 "std::string fourcc;", "std::string orientation", "ck_ingest_create_raw"):
        assert name in src, name


@pytest.mark.gpu
def test_cpp_raw_luma_and_detections(built, tmp_path):
    import scenes
    w, h, f, n = 640, 480, 600.0, 2
    layout = scenes.wall_layout(6, cols=3)
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
    frames = [scenes.render_view(500 + i, w, h, f, layout, (2.0, 0.05 * i, 0.0), r2c, noise_amp=2)[0] for i in range(n)]
    for fourcc, o in (("YUYV", "none"), ("UYVY", "clockwise"), ("BGR3", "rotate-180"), ("RGBA", "counterclockwise")):
        W, H = (h, w) if o in ("clockwise", "counterclockwise") else (w, h)
        src = [R.grey_to_rgb(fr, seed=3) if R.is_colour(fourcc) else fr for fr in frames]
        stride = R.min_stride(fourcc, w) + 5
        packed = np.stack([R.pack(s, fourcc, stride, seed=i) for i, s in enumerate(src)])
        want = np.stack([R.expected(p, fourcc, w, h, stride, o) for p in packed])
        fin, fout = tmp_path / "in.raw", tmp_path / "out.luma"
        packed.tofile(fin)
        r = _run("luma", fourcc, o, W, H, n, stride, fin, fout)
        assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
        got = np.fromfile(fout, np.uint8).reshape(n, H, W)
        assert np.array_equal(got, want), (fourcc, o, int((got != want).sum()))
        # every tag of the wall behind Handle::upload_raw; AprilTags::process with Config::{fourcc, orientation} staged the same luma
        assert r.stdout.split()[1:] == ["6/1"] * n, r.stdout
