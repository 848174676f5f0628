"""The planar 4:2:0 raw formats of the C++ host layer (include/chalkydri.hpp: raw_format's `planes`, raw_plane_layout) through
tests/cpp/raw_planes_demo.cpp: the plane layout without a GPU, and on a GPU one NV12 colour file byte-equal to Python's."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg_enc_color as EC  # noqa: E402
import raw_format_ref as R  # noqa: E402
import raw_planes_ref as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "raw_planes_demo")


def test_raw_planes_demo_layout(built):
    assert os.path.exists(DEMO)
    r = subprocess.run([DEMO], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
    for code in P.FOURCCS:
        for o in R.ORIENTATIONS:
            for (w, h), extra in (((17, 19), 6), ((34, 18), 0)):
                sw, sh = R.source_size(w, h, o)
                stride = P.min_stride(sw) + extra
                r = subprocess.run([DEMO, "layout", code, o, str(w), str(h), str(stride)], capture_output=True, text=True, timeout=60)
                off, rs, st, total = P.formulas(code, sw, sh, stride)
                want = [sw, sh, *P.chroma_size(sw, sh), *off, *rs, *st, total]
                assert r.returncode == 0 and [int(v) for v in r.stdout.split()] == want, (code, o, r.stdout, r.stderr)
    r = subprocess.run([DEMO, "layout", "I420", "clockwise", "17", "19", "24"], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == "19 17 10 9 0 408 516 24 12 12 1 1 1 624".split()
    # the layer's errors: a stride the layout cannot have, a fourcc without planes, an orientation it does not know
    for args in (("NV12", "none", "17", "19", "17"), ("I420", "none", "17", "19", "19"), ("YUYV", "none", "16", "16", "32"),
                 ("NV12", "sideways", "16", "16", "16")):
        r = subprocess.run([DEMO, "layout", *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 3 and "panic" in r.stderr, args


@pytest.mark.gpu
def test_cpp_nv12_colour_file_equals_pythons(built, tmp_path):
    from chalkydri_amd.detector import AprilTagDetector
    W, H, n, o, q = 34, 18, 2, "clockwise", 50
    rng = np.random.default_rng(9)
    sw, sh = R.source_size(W, H, o)
    stride = P.min_stride(sw) + 6
    raw = [P.pack_planes(*P.random_planes(rng, sw, sh), "NV12", stride, pad_byte=None, seed=k) for k in range(n)]
    (tmp_path / "in.bin").write_bytes(b"".join(f.tobytes() for f in raw))
    r = subprocess.run([DEMO, "color", "NV12", o, str(W), str(H), str(stride), str(q), str(n), str(tmp_path / "in.bin"), str(tmp_path / "p")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.split() == ["OK", str(n)], (r.stdout, r.stderr)
    det = AprilTagDetector(W, H, max_batch=n)
    det.upload_raw(raw, "NV12", o, planes=True)
    files = det.preview_jpeg_color(n=n, width=0, height=0, quality=q)
    det.close()
    for i in range(n):
        got = (tmp_path / f"p{i}.jpg").read_bytes()
        assert got == files[i] == EC.encode_ycc(P.triples_vec(raw[i], "NV12", sw, sh, stride, o), q, 0), i
