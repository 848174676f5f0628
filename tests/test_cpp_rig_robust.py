"""The robust camera rig outside Python: the host twin under AddressSanitizer + UBSan (tests/cpp/rig_robust_host_check.cpp, a stand-alone
program of ck_rig_host.c alone) and the C++ host layer (include/chalkydri.hpp: RigSolver::solve_robust) through
tests/cpp/rig_robust_demo.cpp, against Python's RigSolver on the same steps."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_rig as N  # noqa: E402
import np_rig_robust as NR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "rig_robust_demo")
CHECK = os.path.join(ROOT, "chalkydri_amd", "lib", "rig_robust_host_check")


def _case(tmp_path):
    """the 3-camera cases of the suite (outliers of every kind, a camera that sees nothing, clean ones) as the demo reads them, and
    as RigSolver takes them"""
    from chalkydri_amd.sqpnp import iso3
    cases = NR.suite()[3][:6]
    steps, gyros, blob = [], [], [np.int32([len(cases), 3]).tobytes()]
    for c in cases:
        step = []
        for tags, b, (Am, bb) in c["cams"]:
            isos, mount = [iso3(t, N.mat_to_quat(R)) for R, t in tags], iso3(bb, N.mat_to_quat(Am))
            step.append((isos, b, mount))
            blob.append(np.int32(len(tags)).tobytes())
            for i in [mount] + isos:
                blob.append(np.array(list(i.t) + list(i.q), np.float64).tobytes())
            blob.append(np.ascontiguousarray(b, np.float64).tobytes())
        steps.append(step); gyros.append(c["gyro"])
    blob.append(np.array(gyros, np.float64).tobytes())
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    return steps, gyros, [c["planted"] for c in cases]


def test_host_twin_under_sanitizers(built, tmp_path):
    """The suite's 3-camera cases through the sanitized twin: in one batch, every step alone in arrays allocated to the byte, and with
    min_inlier_tags above what the step has; the program exits non-zero on the first finding of either sanitizer.  Its records are
    the library's."""
    from chalkydri_amd.rig import RigSolver
    steps, gyros, _ = _case(tmp_path)
    sym = subprocess.run(["nm", CHECK], capture_output=True, text=True).stdout
    assert "__asan_init" in sym and "__ubsan_handle" in sym          # the build that ran is the sanitized one
    r = subprocess.run([CHECK, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK 6 steps"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert (tmp_path / "out.bin").read_bytes() == RigSolver().solve_host(steps, gyros, robust=True).tobytes()


def test_cpp_solve_robust_host(built, tmp_path):
    """chalkydri::RigSolver::solve_robust on the host returns the bytes of Python's RigSolver.solve_host(robust=True)"""
    from chalkydri_amd.rig import RigSolver
    steps, gyros, planted = _case(tmp_path)
    r = subprocess.run([DEMO, "host", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[0] == "OK", (r.stdout, r.stderr)
    want = RigSolver().solve_host(steps, gyros, robust=True)
    assert want["fused"]["valid"].all() and [[int(m) for m in w["rejected"][:3]] for w in want] == planted
    assert r.stdout.split() == ["OK", "6", "of", "6,", str(int(want["n_rejected"].sum())), "rejected"] and want["n_rejected"].sum() >= 3
    assert (tmp_path / "out.bin").read_bytes() == want.tobytes()
    r = subprocess.run([DEMO, "nonsense", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "unknown mode" in r.stderr


@pytest.mark.gpu
def test_cpp_solve_robust_batch(built, tmp_path):
    """... and on a handle of its own the bytes of Python's solve_batch(robust=True)"""
    from chalkydri_amd.detector import AprilTagDetector
    from chalkydri_amd.rig import RigSolver
    steps, gyros, planted = _case(tmp_path)
    r = subprocess.run([DEMO, "batch", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "OK", (r.stdout, r.stderr)
    det = AprilTagDetector(64, 64)
    want = RigSolver(det).solve_batch(steps, gyros, robust=True)
    det.close()
    assert [[int(m) for m in w["rejected"][:3]] for w in want] == planted
    assert (tmp_path / "out.bin").read_bytes() == want.tobytes()
