"""The camera rig outside Python: the host twin under AddressSanitizer + UBSan (tests/cpp/rig_host_check.cpp, a stand-alone program of
ck_rig_host.c alone) and the C++ host layer (include/chalkydri.hpp: RigSolver) through tests/cpp/rig_demo.cpp."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_rig as N  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "chalkydri_amd", "lib")
DEMO, CHECK = os.path.join(LIB, "rig_demo"), os.path.join(LIB, "rig_host_check")


def test_host_twin_under_sanitizers(built):
    """20 random rigs of 1..4 cameras against their truth, one camera at offsets inside larger arrays, a step without tags, no steps,
    and the refusals: the program exits non-zero on the first finding of either sanitizer."""
    assert os.path.exists(CHECK)
    sym = subprocess.run(["nm", CHECK], capture_output=True, text=True).stdout
    assert "__asan_init" in sym and "__ubsan_handle" in sym          # the build that ran is the sanitized one
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK 20 rigs"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def _case(tmp_path):
    """6 steps of 3 cameras (a camera may see nothing) as rig_demo reads them, and as RigSolver takes them"""
    from chalkydri_amd.sqpnp import iso3
    rng = np.random.default_rng(8)
    steps, gyros, blob = [], [], [np.int32([6, 3]).tobytes()]
    for _ in range(6):
        cams, gyro, _ = N.make_rig(rng, n_cams=3, noise=1e-3, gyro_noise=0.02)
        step = []
        for tags, b, (Am, bb) in cams:
            isos, mount = [iso3(t, N.mat_to_quat(R)) for R, t in tags], iso3(bb, N.mat_to_quat(Am))
            step.append((isos, b, mount))
            blob.append(np.int32(len(tags)).tobytes())
            for i in [mount] + isos:
                blob.append(np.array(list(i.t) + list(i.q), np.float64).tobytes())
            blob.append(np.ascontiguousarray(b, np.float64).tobytes())
        steps.append(step); gyros.append(gyro)
    blob.append(np.array(gyros, np.float64).tobytes())
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    return steps, gyros


def test_cpp_rig_solver_host(built, tmp_path):
    """chalkydri::RigSolver::solve_host returns the bytes of Python's RigSolver.solve_host (no device on either side)."""
    from chalkydri_amd.rig import RigSolver
    steps, gyros = _case(tmp_path)
    r = subprocess.run([DEMO, "host", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[0] == "OK", (r.stdout, r.stderr)
    want = RigSolver().solve_host(steps, gyros)
    assert want["valid"].all() and (tmp_path / "out.bin").read_bytes() == want.tobytes()
    r = subprocess.run([DEMO, "nonsense", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "unknown mode" in r.stderr


@pytest.mark.gpu
def test_cpp_rig_solver_batch(built, tmp_path):
    """... and RigSolver::solve_batch, on a handle of its own, the bytes of Python's solve_batch."""
    from chalkydri_amd.detector import AprilTagDetector
    from chalkydri_amd.rig import RigSolver
    steps, gyros = _case(tmp_path)
    r = subprocess.run([DEMO, "batch", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "OK", (r.stdout, r.stderr)
    det = AprilTagDetector(64, 64)
    want = RigSolver(det).solve_batch(steps, gyros)
    det.close()
    assert want["valid"].all() and (tmp_path / "out.bin").read_bytes() == want.tobytes()


@pytest.mark.gpu
def test_cpp_rig_process_last(built, tmp_path):
    """chalkydri::rig_process_last behind two AprilTags::process calls returns the bytes of Python's AprilTagsRig.process_batch: two
    cameras of different size on one robot, three instants, one of them without a gyro heading."""
    import scenes
    from chalkydri_amd.apriltags import AprilTags
    from chalkydri_amd.rig import AprilTagsRig
    from test_gpu_rig import CAMS
    layout = scenes.wall_layout(12)
    poses = [(1.8, 0.2, 0.1), (2.2, -0.3, -0.15), (1.6, 0.0, 0.05)]
    gyro = [poses[0][2] + 0.01, None, poses[2][2] - 0.01]
    blob, frames, tasks = [np.int32(3).tobytes()], [], []
    for c, (w, h, f, r2c) in enumerate(CAMS):
        fr = np.stack([scenes.render_view(3000 + 10 * i + c, w, h, f, layout, p, r2c, noise_amp=1)[0] for i, p in enumerate(poses)])
        frames.append(fr)
        blob += [np.int32([w, h]).tobytes(), np.float64([f, r2c["x"], r2c["y"], r2c["z"], r2c["roll"], r2c["pitch"], r2c["yaw"]]).tobytes(), fr.tobytes()]
        tasks.append(AprilTags(w, h, layout, scenes.pinhole_calib(f, w / 2.0, h / 2.0), r2c, cam_id=c, max_batch=3))
    blob += [np.float64([g or 0.0 for g in gyro]).tobytes(), np.int32([g is not None for g in gyro]).tobytes()]
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    r = subprocess.run([DEMO, "last", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["OK", "2", "of", "3"], (r.stdout, r.stderr)
    rig = AprilTagsRig(tasks, rig_id=42)
    recs, valid, _ = rig.process_batch(frames, gyro)
    for t in tasks:
        t.detector.close()
    assert list(valid) == [True, False, True]
    assert (tmp_path / "out.bin").read_bytes() == bytes(recs) + valid.astype(np.int32).tobytes() + rig.last_results.tobytes()
