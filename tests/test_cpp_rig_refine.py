"""The rig pose refinement through the C++ host layer (include/chalkydri.hpp: RigSolver::refine) in tests/cpp/rig_refine_demo.cpp,
against Python's RigSolver on the same steps: the robust solve, then the refinement with its masks and a heading prior."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpp_rig_robust import _case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "rig_refine_demo")


def _params():
    from chalkydri_amd.rig import RefineParams
    return RefineParams(gyro_sigma=0.01, max_iters=30)


def test_cpp_refine_host(built, tmp_path):
    """chalkydri::RigSolver::refine on the host returns the bytes of Python's RigSolver.refine_host on the robust records"""
    from chalkydri_amd import _abi as A
    from chalkydri_amd.rig import RigSolver
    steps, gyros, planted = _case(tmp_path)
    r = subprocess.run([DEMO, "host", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[0] == "OK", (r.stdout, r.stderr)
    s = RigSolver()
    rob = s.solve_host(steps, gyros, robust=True)
    want = s.refine_host(steps, gyros, rob, _params())
    assert (want["status"] <= A.CK_RIG_REFINE_MAXITERS).all() and (want["n_points"] == 4 * rob["fused"]["n_tags"]).all() and rob["n_rejected"].sum() >= 3
    assert r.stdout.split() == ["OK", "6", "of", "6"]
    assert (tmp_path / "out.bin").read_bytes() == want.tobytes()
    # no prior: the C++ layer takes no headings at all, as the C call takes a null gyro
    from chalkydri_amd.rig import RefineParams
    r = subprocess.run([DEMO, "host_no_heading", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[0] == "OK", (r.stdout, r.stderr)
    assert (tmp_path / "out.bin").read_bytes() == s.refine_host(steps, None, rob["fused"], RefineParams(max_iters=30)).tobytes()
    r = subprocess.run([DEMO, "nonsense", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "unknown mode" in r.stderr


@pytest.mark.gpu
def test_cpp_refine_batch(built, tmp_path):
    """... and on a handle of its own the bytes of Python's solve_batch(robust=True), then refine_batch"""
    from chalkydri_amd.detector import AprilTagDetector
    from chalkydri_amd.rig import RigSolver
    steps, gyros, planted = _case(tmp_path)
    r = subprocess.run([DEMO, "batch", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "OK", (r.stdout, r.stderr)
    det = AprilTagDetector(64, 64)
    s = RigSolver(det)
    want = s.refine_batch(steps, gyros, s.solve_batch(steps, gyros, robust=True), _params())
    det.close()
    assert (tmp_path / "out.bin").read_bytes() == want.tobytes()
