"""The colour preview of the C++ host layer (include/chalkydri.hpp: preview_jpeg_color, IngestRing::preview_jpeg_color) through
tests/cpp/preview_color_demo.cpp: on a GPU the files byte-equal to the numpy restatement (tests/np_jpeg_enc_color.py), from the
handle's raw staging and from a slot of a raw ring."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg_enc_color as EC  # noqa: E402
import preview_color_ref as PC  # noqa: E402
import raw_format_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "preview_color_demo")


def test_preview_color_demo_is_built(built):
    assert os.path.exists(DEMO)
    r = subprocess.run([DEMO], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "ring"])
def test_cpp_preview_color_files(built, tmp_path, form):
    W, H, n = 66, 49, 3
    rng = np.random.default_rng(6)
    for fourcc, o, (width, height), q, rr in (("YUYV", "clockwise", (0, 0), 50, 0), ("BGR3", "rotate-180", (37, 21), 85, 1)):
        sw, sh = R.source_size(W, H, o)
        raw = [PC.pack_colour(rng, fourcc, sw, sh) for _ in range(n)]
        (tmp_path / "in.bin").write_bytes(b"".join(f.tobytes() for f in raw))
        r = subprocess.run([DEMO, form, fourcc, str(R.ORIENT_CODE[o]), str(width), str(height), str(q), str(rr), str(W), str(H), str(n),
                            str(tmp_path / "in.bin"), str(tmp_path / "p")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.split() == ["OK", str(n)], (r.stdout, r.stderr)
        pw, ph, _ = EC.layout(width, height, W, H, q, rr)
        for i in range(n):
            want = EC.encode_ycc(PC.triples_vec(raw[n - 1 - i], fourcc, sw, sh, R.min_stride(fourcc, sw), o, pw, ph), q, rr)
            assert (tmp_path / f"p{i}.jpg").read_bytes() == want, (form, fourcc, i)
