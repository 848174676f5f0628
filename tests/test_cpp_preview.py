"""The preview entry points of the C++ host layer (include/chalkydri.hpp: preview_params, preview_jpeg, preview_luma, mjpeg_part)
through tests/cpp/preview_demo.cpp: the layout and the multipart framing without a GPU, and on a GPU the files byte-equal to the
numpy restatement (tests/np_jpeg_enc.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg_enc as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "preview_demo")


def _run(*args):
    return subprocess.run([DEMO, *map(str, args)], capture_output=True, text=True, timeout=600)


def test_preview_demo_layout_and_framing_need_no_gpu(built, tmp_path):
    assert os.path.exists(DEMO)
    for width, height, q, rr, W, H in ((640, 480, 50, 0, 1280, 800), (640, 480, 50, 1, 272, 200), (0, 0, 100, 3, 641, 479), (8, 8, 1, 0, 16, 16)):
        r = _run("layout", width, height, q, rr, W, H)
        assert r.returncode == 0 and tuple(int(v) for v in r.stdout.split()) == E.layout(width, height, W, H, q, rr), (r.stdout, r.stderr)
    assert _run("layout", 7, 480, 50, 0, 640, 480).returncode == 3           # a Panic, as every refused call of the layer
    assert _run("layout", 640, 480, 101, 0, 640, 480).returncode == 3
    j = E.encode_grey(np.arange(64, dtype=np.uint8).reshape(8, 8))
    (tmp_path / "in.jpg").write_bytes(j)
    assert _run("part", tmp_path / "in.jpg", tmp_path / "out.bin").returncode == 0
    assert (tmp_path / "out.bin").read_bytes() == E.mjpeg_part(j)


@pytest.mark.gpu
def test_cpp_preview_files(built, tmp_path):
    import scenes
    W, H, n = 640, 480, 3
    F = scenes.bench_stream(4, n, W, H, 4)[0]
    (tmp_path / "in.bin").write_bytes(np.ascontiguousarray(F).tobytes())
    for width, height, q, rr in ((640, 480, 50, 0), (320, 200, 85, 1), (333, 77, 20, 3)):
        r = _run("jpeg", width, height, q, rr, W, H, n, tmp_path / "in.bin", str(tmp_path / "p"))
        assert r.returncode == 0 and r.stdout.split() == ["OK", str(n)], (r.stdout, r.stderr)
        pw, ph, _ = E.layout(width, height, W, H, q, rr)
        for i in range(n):
            assert (tmp_path / f"p{i}.jpg").read_bytes() == E.encode_grey(E.scale_nn(F[n - 1 - i], pw, ph), q, rr), (width, height, i)
