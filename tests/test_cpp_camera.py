"""The camera models outside Python: the C++ host layer (include/chalkydri.hpp: Camera, Handle::set_camera, AprilTags::Config::camera,
Calibrator::calibrate(CameraModel)) through tests/cpp/camera_demo.cpp returns the bytes of the Python layer."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_camera as NC  # noqa: E402
import np_camera_calib as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "camera_demo")


def _run(*args):
    return subprocess.run([DEMO, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_cpp_camera_matches_python(built, tmp_path):
    """Camera::eucm / ucm, unproject and project: the bytes of chalkydri_amd.camera's host functions, invalid pixels among them; a
    camera that ck_camera_check refuses is a Panic."""
    from chalkydri_amd import camera
    px = np.concatenate([NC.grid(64), [[3000.0, 400.0], [-900.0, -900.0]]])
    (tmp_path / "px.bin").write_bytes(px.tobytes())
    for name, lens in (("eucm", NC.LENSES["eucm_wide"]), ("ucm", NC.LENSES["ucm"])):
        r = _run("model", name, *lens, tmp_path / "px.bin", tmp_path / "out.bin")
        assert r.returncode == 0 and r.stdout.split() == ["OK", str(len(px))], (r.stdout, r.stderr)
        c = camera.make_camera("UCM", *lens[:5]) if name == "ucm" else camera.make_camera("EUCM", *lens)
        b, ok = camera.unproject_host(c, px)
        back, _ = camera.project(c, b)
        assert not ok.all() and ok.sum() >= len(px) - 2
        assert (tmp_path / "out.bin").read_bytes() == b.tobytes() + ok.astype(np.uint8).tobytes() + back.tobytes()
    r = _run("model", "eucm", 500, 502, 640, 400, 1.5, 1.08, tmp_path / "px.bin", tmp_path / "out.bin")
    assert r.returncode == 3 and "ck_camera_check" in r.stderr


@pytest.mark.gpu
def test_cpp_calibrator_camera_models(built, tmp_path):
    """Calibrator::add_observations + calibrate(CameraModel) return the bytes of Python's camera_calibrate_batch."""
    from chalkydri_amd import calibration as K
    from chalkydri_amd.detector import AprilTagDetector
    det = AprilTagDetector(NC.W, NC.H)
    for name, model, mask in (("eucm_wide", "EUCM", 0), ("ucm", "UCM", 0), ("eucm_wide", "EUCM", 1 << 5)):
        frames, _ = M.make_case(NC.LENSES[name], 4, 0.1, 1)
        b = np.concatenate([f[0] for f in frames])
        u = np.concatenate([f[1] for f in frames])
        s = np.concatenate([[0], np.cumsum([len(f[0]) for f in frames])]).astype(np.int32)
        (tmp_path / "in.bin").write_bytes(np.int32(4).tobytes() + s.tobytes() + b.tobytes() + u.tobytes())
        r = _run("points", NC.W, NC.H, model.lower(), mask, tmp_path / "in.bin", tmp_path / "out.bin")
        assert r.returncode == 0 and r.stdout.split()[0] == "OK", (r.stdout, r.stderr)
        res, poses = K.camera_calibrate_batch(det, model, K.params(NC.W, NC.H, fixed_mask=mask), [frames])
        assert (tmp_path / "out.bin").read_bytes() == res.tobytes() + poses[0].tobytes(), (name, mask)
    det.close()
    (tmp_path / "in.bin").write_bytes(np.int32(2).tobytes() + s[:3].tobytes() + b[:s[2]].tobytes() + u[:s[2]].tobytes())
    r = _run("points", NC.W, NC.H, "eucm", 0, tmp_path / "in.bin", tmp_path / "out.bin")
    assert r.returncode == 0 and r.stdout.split()[0] == "NONE"               # fewer than min_frames frames: no model, no panic


@pytest.mark.gpu
def test_cpp_task_with_a_camera(built, tmp_path):
    """AprilTags::Config::camera: the task's measurement is the Python task's with the same EUCM blob, byte for byte."""
    import scenes
    from chalkydri_amd.apriltags import AprilTags
    w, h, f = 640, 480, 576.0
    layout = scenes.wall_layout(6, cols=3)
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
    frame, _ = scenes.render_view(71, w, h, f, layout, (2.2, 0.1, 0.05), r2c, noise_amp=1)
    (tmp_path / "frame.bin").write_bytes(frame.tobytes())
    task = AprilTags(w, h, layout, {"EUCM": dict(fx=f, fy=f, cx=w / 2.0, cy=h / 2.0, alpha=0.3, beta=1.2)}, r2c, cam_id=3)
    recs, valid = task.process_batch(frame[None], [0.05])
    task.detector.close()
    r = _run("process", w, h, f, 0.3, 1.2, tmp_path / "frame.bin")
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = r.stdout.split()
    assert out[:4] == ["VALID", str(int(valid[0])), "TAGS", str(recs[0].tag_count)] and valid[0] and out[4] == bytes(recs[0]).hex()
