"""The camera calibration outside Python: the host half under AddressSanitizer + UBSan (tests/cpp/calib_host_check.cpp, a stand-alone
program of ck_calib_host.c alone) and the C++ host layer (include/chalkydri.hpp: Board, Calibrator) through tests/cpp/calib_demo.cpp."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_calib as N  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "chalkydri_amd", "lib")
DEMO, CHECK = os.path.join(LIB, "calib_demo"), os.path.join(LIB, "calib_host_check")


def test_host_half_under_sanitizers(built):
    """init, the host refinement (whole arrays, offsets, in place, frozen parameters, MAXIT) and the refusals on one F = 4 case: the
    program exits non-zero on the first finding of either sanitizer."""
    assert os.path.exists(CHECK)
    sym = subprocess.run(["nm", CHECK], capture_output=True, text=True).stdout
    assert "__asan_init" in sym and "__ubsan_handle" in sym          # the build that ran is the sanitized one
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_cpp_board_matches_python(built, tmp_path):
    from chalkydri_amd.calibration import Board
    for args in ((6, 6, 0.088, 0.3, 0), (2, 5, 0.1, 0.25, 7)):
        r = subprocess.run([DEMO, "board", *map(str, args), str(tmp_path / "b.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 3 and "no such tag" in r.stderr            # the demo ends by asking for a tag past the board: a Panic
        got = np.frombuffer((tmp_path / "b.bin").read_bytes(), np.float64).reshape(-1, 2)
        assert np.array_equal(got, Board(*args).points())


@pytest.mark.gpu
def test_cpp_calibrator_points(built, tmp_path):
    """Calibrator::add_observations + calibrate return the bytes of Python's calibrate_batch; calibrate clears the frames."""
    from chalkydri_amd import calibration as K
    from chalkydri_amd.detector import AprilTagDetector
    k, w, h = N.cameras()["cam1_1600x1304"]
    frames, _ = N.make_case(k, w, h, 4, 0.1, 1)
    b, u, s = N.pack(frames)
    (tmp_path / "in.bin").write_bytes(np.int32(4).tobytes() + s.tobytes() + b.tobytes() + u.tobytes())
    det = AprilTagDetector(w, h)
    for mask in (0, K.FIX_DISTORTION):
        r = subprocess.run([DEMO, "points", str(w), str(h), str(mask), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.split()[0] == "OK", (r.stdout, r.stderr)
        res, poses = K.calibrate_batch(det, K.params(w, h, fixed_mask=mask), [frames])
        assert (tmp_path / "out.bin").read_bytes() == res.tobytes() + poses[0].tobytes(), mask
    det.close()
    (tmp_path / "in.bin").write_bytes(np.int32(2).tobytes() + s[:3].tobytes() + b[:s[2]].tobytes() + u[:s[2]].tobytes())
    r = subprocess.run([DEMO, "points", str(w), str(h), "0", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "NONE"               # fewer than min_frames frames: no model, no panic
