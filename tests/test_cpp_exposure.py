"""The exposure entry points of the C++ host layer (include/chalkydri.hpp: exposure_params, exposure_stats, ExposureController)
through tests/cpp/exposure_demo.cpp: the tables, the controller and the region of interest without a GPU, and on a GPU the records
byte-equal to the numpy restatement (tests/np_exposure.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_exposure as N  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "exposure_demo")


def _run(*args):
    return subprocess.run([DEMO, *map(str, args)], capture_output=True, text=True, timeout=600)


def test_exposure_demo_host_arithmetic_needs_no_gpu(built, tmp_path):
    assert os.path.exists(DEMO)
    assert _run("luts", tmp_path / "lut.bin").returncode == 0
    from chalkydri_amd.exposure import ExposureParams
    assert (tmp_path / "lut.bin").read_bytes() == ExposureParams().luts().tobytes()
    rng = np.random.default_rng(3)
    s = N.stats(np.clip(60 + rng.integers(-40, 41, (48, 64)), 0, 255).astype(np.uint8), N.luts())
    (tmp_path / "s.bin").write_bytes(s.tobytes())
    r = _run("recommend", tmp_path / "s.bin", 2.5, 3)
    assert r.returncode == 0, r.stderr
    e, p = 2.5, N.Params()
    for line in r.stdout.splitlines():
        e, g = N.recommend(p, s, e)
        got = [float(v) for v in line.split()]
        assert abs(got[0] - e) <= 1e-12 * e and abs(got[1] - g) <= 1e-12 * g
    assert _run("recommend", tmp_path / "s.bin", -1, 1).returncode == 3          # a Panic, as every refused call of the layer
    from chalkydri_amd.exposure import roi_from_detections
    assert _run("roi", 640, 480, 8).stdout.split() == ["0", "0", "640", "480"]
    corners = [100.5, 50.2, 140.9, 52.0, 139.0, 90.7, 99.1, 88.0]

    class D:
        def corners(self):
            return np.array(corners).reshape(4, 2)
    assert tuple(int(v) for v in _run("roi", 640, 480, 8, *corners).stdout.split()) == roi_from_detections([D()], 8, 640, 480)


@pytest.mark.gpu
def test_cpp_exposure_stats(built, tmp_path):
    import scenes
    W, H, n = 640, 480, 3
    F = scenes.bench_stream(4, n, W, H, 4)[0]
    (tmp_path / "in.bin").write_bytes(np.ascontiguousarray(F).tobytes())
    lut = N.luts()
    for roi in (None, (100, 37, 601, 470)):
        r = _run("stats", W, H, n, tmp_path / "in.bin", tmp_path / "out.bin", *(roi or ()))
        assert r.returncode == 0 and r.stdout.split() == ["OK", str(n)], (r.stdout, r.stderr)
        got = np.frombuffer((tmp_path / "out.bin").read_bytes(), N.STATS_DTYPE)
        for i in range(n):
            assert got[i].tobytes() == N.stats(F[n - 1 - i], lut, roi).tobytes(), (roi, i)
