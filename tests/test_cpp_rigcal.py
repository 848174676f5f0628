"""The mount calibration outside Python: the host half under AddressSanitizer + UBSan (tests/cpp/rigcal_host_check.cpp, a stand-alone
program of ck_rigcal_host.c alone, run as a program) and the C++ host layer (include/chalkydri.hpp: MountCalibrator) through
tests/cpp/rigcal_demo.cpp, byte-equal to Python on the host and, on a handle of its own, on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "chalkydri_amd", "lib", "rigcal_host_check")
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "rigcal_demo")


def test_host_half_under_sanitizers(built):
    """random captures of 2 and 3 cameras against their truth (skipped one-camera steps, a camera absent from some steps), a subset at
    offsets inside larger arrays with a frozen position and MAXIT, the Jacobian's frozen columns and every refusal of ck_rigcal_check in
    its order: the program exits non-zero on the first finding of either sanitizer."""
    assert os.path.exists(CHECK)
    sym = subprocess.run(["nm", CHECK], capture_output=True, text=True).stdout
    assert "__asan_init" in sym and "__ubsan_handle" in sym          # the build that ran is the sanitized one
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- the C++ host layer ----------------------------------------------------------------------------------------------------------------
def _case_file(path, case, gyro, mask, max_iters):
    """the capture as rigcal_demo reads it"""
    out = [np.array([case["n_cams"], case["n_steps"], max_iters, 0], np.int32).tobytes(), np.uint64(mask).tobytes()]
    out += [bytes(m) for m in case["m0"]]
    for s, cams in enumerate(case["csteps"]):
        out += [np.float64(gyro[s]).tobytes(), case["poses0"][s].tobytes()]
        for tags, bear in cams:
            out += [np.int32(len(tags)).tobytes()] + [bytes(t) for t in tags] + [np.ascontiguousarray(bear, np.float64).tobytes()]
    path.write_bytes(b"".join(out))


def _run(mode, tmp_path, word="OK"):
    r = subprocess.run([DEMO, mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == word, (r.stdout, r.stderr)
    return (tmp_path / "out.bin").read_bytes()


def test_cpp_host_refinement_matches_python(built, tmp_path):
    """MountCalibrator::refine on the host returns the bytes of Python's refine_host: all free, and a frozen position with three
    iterations"""
    import rigcal_cases as RC
    from chalkydri_amd import rigcal as K
    case = RC.shape_case(5, 3, 9, lambda s, c: 0 if (c == 2 and s % 3 == 0) else 1 + (s + c) % 2)
    for mask, max_iters in ((0x3F, 100), (0x3F | K.fix_position(1), 3)):
        _case_file(tmp_path / "in.bin", case, np.zeros(9), mask, max_iters)
        res, poses = K.refine_host(K.params(mask, max_iters=max_iters), K.Capture(case["csteps"]), case["m0"], case["poses0"])
        assert _run("host", tmp_path, "OK" if max_iters == 100 else "NONE") == res.tobytes() + poses.tobytes(), mask   # (MAXIT: no mounts)


@pytest.mark.gpu
def test_cpp_batch_matches_python(built, tmp_path):
    """the C++ layer on a handle of its own: refine on the device and calibrate (starts from the rig solver) return the bytes of
    Python's refine_batch and calibrate_batch"""
    import rigcal_cases as RC
    from chalkydri_amd import rigcal as K
    from chalkydri_amd.detector import AprilTagDetector
    cs = RC.acceptance_case(3, 12, 2, 1e-3)
    case = {"n_cams": 3, "n_steps": 12, "m0": cs["m0"], "csteps": cs["csteps"], "poses0": cs["poses0"]}
    gyro = [np.arctan2(R[0, 1], R[0, 0]) for R, _ in cs["truth"]]
    _case_file(tmp_path / "in.bin", case, gyro, 0x3F, 100)
    det = AprilTagDetector(64, 64)
    p, cap = K.params(0x3F), K.Capture(cs["csteps"])
    res, poses = K.refine_batch(det, p, cap, cs["m0"], cs["poses0"])
    assert _run("batch", tmp_path) == res[0].tobytes() + poses[0].tobytes()
    res, poses = K.calibrate_batch(det, p, cap, cs["m0"], gyro)
    assert _run("calibrate", tmp_path) == res[0].tobytes() + poses[0].tobytes()
    det.close()
