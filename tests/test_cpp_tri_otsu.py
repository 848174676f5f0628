"""The tri-class threshold of the C++ host layer (include/chalkydri.hpp: tri_otsu_params, tri_otsu_solve, apriltags::Detector::tri_otsu)
through tests/cpp/tri_otsu_demo.cpp: the solve without a GPU, and on a GPU the record and the class map byte-equal to the
restatement (tests/np_tri_otsu.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_tri_otsu as N  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "tri_otsu_demo")


def _run(*args):
    return subprocess.run([DEMO, *map(str, args)], capture_output=True, text=True, timeout=600)


def test_tri_otsu_demo_solve_needs_no_gpu(built, tmp_path):
    assert os.path.exists(DEMO)
    rng = np.random.default_rng(9)
    g = np.arange(256)
    hists = [np.floor(5000 * np.exp(-0.5 * ((g - 70) / 18.0) ** 2) + 3000 * np.exp(-0.5 * ((g - 190) / 25.0) ** 2)).astype(np.uint32),
             rng.integers(0, 1 << 16, 256).astype(np.uint32), np.zeros(256, np.uint32)]
    for i, h in enumerate(hists):
        (tmp_path / "h.bin").write_bytes(h.tobytes())
        for args, kw in (((), {}), ((3, 2, 0), {"max_iters": 3, "min_delta": 2, "keep_tbd": 0})):
            r = _run("solve", tmp_path / "h.bin", tmp_path / "o.bin", *args)
            assert r.returncode == 0, r.stderr
            info, lut = N.solve(h, **kw)
            assert (tmp_path / "o.bin").read_bytes() == info.tobytes() + lut.tobytes(), (i, kw)
    assert _run("solve", tmp_path / "h.bin", tmp_path / "o.bin", 0, 1, 1).returncode == 3      # a Panic, as every refused call of the layer
    assert _run("solve", tmp_path / "h.bin", tmp_path / "o.bin", 8, 1, 2).returncode == 3


@pytest.mark.gpu
def test_cpp_detector_tri_otsu(built, tmp_path):
    from chalkydri_amd import synth
    w, h = 130, 67
    g = synth.render(synth.frame_seed(5, 3), 320, 240, 3, min_side=40, max_side=110, noise_amp=2)[0][60:60 + h, 40:40 + w]
    for ch, keep in ((3, 1), (1, 0)):
        f = np.ascontiguousarray(np.repeat(g[..., None], ch, axis=2))
        (tmp_path / "in.bin").write_bytes(f.tobytes())
        r = _run("frame", w, h, ch, keep, tmp_path / "in.bin", tmp_path / "out.bin")
        assert r.returncode == 0 and r.stdout.split()[0] == "OK", (r.stdout, r.stderr)
        cls, info, _ = N.classify(f, keep_tbd=keep)
        assert (tmp_path / "out.bin").read_bytes() == info.tobytes() + cls.tobytes(), (ch, keep)
    (tmp_path / "in.bin").write_bytes(b"\0" * 10)
    assert _run("frame", w, h, 3, 1, tmp_path / "in.bin", tmp_path / "out.bin").returncode == 3
