"""The field calibration outside Python: the host half under AddressSanitizer + UBSan (tests/cpp/fieldcal_host_check.cpp, a
stand-alone program of ck_fieldcal_host.c and ck_rigcal_host.c alone, run as a program) and the C++ host layer (include/chalkydri.hpp:
FieldCalibrator) through tests/cpp/fieldcal_demo.cpp, byte-equal to Python on the host and, on a handle of its own, on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "chalkydri_amd", "lib", "fieldcal_host_check")
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "fieldcal_demo")


def test_host_half_under_sanitizers(built):
    """random captures of 1 and 3 cameras over a layout of 9 tags against their truth (skipped one-tag steps, a tag seen by several
    cameras, a camera absent from some steps, a layout entry never seen), a subset at offsets inside larger arrays with frozen parts and
    MAXIT, the Jacobian's frozen columns, every refusal of ck_fieldcal_check in its order and both caps: the program exits non-zero
    on the first finding of either sanitizer."""
    assert os.path.exists(CHECK)
    sym = subprocess.run(["nm", CHECK], capture_output=True, text=True).stdout
    assert "__asan_init" in sym and "__ubsan_handle" in sym          # the build that ran is the sanitized one
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- the C++ host layer ----------------------------------------------------------------------------------------------------------------
def _case_file(path, case, gyro, max_iters):
    """the capture as fieldcal_demo reads it"""
    out = [np.array([case["n_cams"], case["n_steps"], len(case["lay0"]), max_iters], np.int32).tobytes()]
    out += [bytes(m) for m in case["m_iso"]] + [bytes(t) for t in case["lay0"]] + [np.asarray(case["fixed"], np.uint8).tobytes()]
    for s, cams in enumerate(case["steps"]):
        out += [np.float64(gyro[s]).tobytes(), case["poses0"][s].tobytes()]
        for ids, bear in cams:
            out += [np.int32(len(ids)).tobytes(), np.asarray(ids, np.int32).tobytes(), np.ascontiguousarray(bear, np.float64).tobytes()]
    path.write_bytes(b"".join(out))


def _run(mode, tmp_path, word="OK"):
    r = subprocess.run([DEMO, mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == word, (r.stdout, r.stderr)
    return (tmp_path / "out.bin").read_bytes()


def _bytes(out, i=None):
    return b"".join((o if i is None else o[i]).tobytes() for o in out)


def test_cpp_host_refinement_matches_python(built, tmp_path):
    """FieldCalibrator::refine on the host returns the bytes of Python's refine_host: one free problem, and partial masks with three
    iterations"""
    import fieldcal_cases as FC
    from chalkydri_amd import fieldcal as K
    for masks, max_iters in (({0: 63}, 100), ({0: 63, 1: 0x38, 2: 0x07}, 3)):
        case = FC.shape_case(5, 3, 9, 6, lambda s, c: [] if (c == 2 and s % 3 == 0) else [(s + c + j) % 5 for j in range(1 + (s + c) % 2)], masks=masks)
        _case_file(tmp_path / "in.bin", case, np.zeros(9), max_iters)
        want = K.refine_host(K.params(max_iters=max_iters), K.Capture(case["steps"]), case["m_iso"], case["lay0"], case["fixed"], case["poses0"])
        assert _run("host", tmp_path, "OK" if max_iters == 100 else "NONE") == _bytes(want), masks     # (MAXIT: no layout)


@pytest.mark.gpu
def test_cpp_batch_matches_python(built, tmp_path):
    """the C++ layer on a handle of its own: refine on the device and calibrate (starts from the rig solver) return the bytes of
    Python's refine_batch and calibrate_batch"""
    import fieldcal_cases as FC
    from chalkydri_amd import fieldcal as K
    from chalkydri_amd.detector import AprilTagDetector
    cs = FC.acceptance_case(2, 40, 1, 1e-3)
    _case_file(tmp_path / "in.bin", cs, cs["gyro"], 100)
    det = AprilTagDetector(64, 64)
    p, cap = K.params(), K.Capture(cs["steps"])
    assert _run("batch", tmp_path) == _bytes(K.refine_batch(det, p, cap, cs["m_iso"], cs["lay0"], cs["fixed"], cs["poses0"]), 0)
    assert _run("calibrate", tmp_path) == _bytes(K.calibrate_batch(det, p, cap, cs["m_iso"], cs["lay0"], cs["fixed"], cs["gyro"]), 0)
    det.close()
