"""Sub-pixel corners outside Python: the C++ host layer (include/chalkydri.hpp: corner_subpix, corner_subpix_host,
Handle::set_corner_subpix, board_corners, Calibrator(recover)) through tests/cpp/subpix_demo.cpp returns the bytes of the Python layer."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subpix_scenes as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "subpix_demo")


def _run(*args):
    return subprocess.run([DEMO, *map(str, args)], capture_output=True, text=True, timeout=300)


def _case(tmp_path):
    frames = np.stack([SC.board_frame(2, 0.8)[0], SC.board_frame(0, 0.8)[0]])
    rng = np.random.default_rng(3)
    fr = rng.integers(0, 2, 80).astype(np.int32)
    truth = [SC.board_frame(2, 0.8)[1]["uv"].reshape(-1, 2), SC.board_frame(0, 0.8)[1]["uv"].reshape(-1, 2)]
    xy = np.array([truth[f][rng.integers(0, 64)] for f in fr]) + rng.uniform(-1.5, 1.5, (80, 2))
    xy[::7] = rng.uniform([0, 0], [SC.W, SC.H], (len(xy[::7]), 2))
    (tmp_path / "frames.bin").write_bytes(frames.tobytes())
    (tmp_path / "points.bin").write_bytes(np.int32(80).tobytes() + fr.tobytes() + xy.tobytes())
    return frames, fr, xy


def test_cpp_host_refinement_matches_python(built, tmp_path):
    from chalkydri_amd import subpix
    frames, fr, xy = _case(tmp_path)
    for w in (3, 5):
        r = _run("host", SC.W, SC.H, 2, w, tmp_path / "frames.bin", tmp_path / "points.bin", tmp_path / "out.bin")
        assert r.returncode == 0 and r.stdout.split() == ["OK", "80"], (r.stdout, r.stderr)
        out, info = subpix.corner_subpix_host(frames, fr, xy, subpix.subpix_params(half_win=w), return_info=True)
        assert (tmp_path / "out.bin").read_bytes() == out.tobytes() + info.tobytes()
    r = _run("host", SC.W, SC.H, 2, 9, tmp_path / "frames.bin", tmp_path / "points.bin", tmp_path / "out.bin")
    assert r.returncode == 3 and "ck_corner_subpix_host" in r.stderr


@pytest.mark.gpu
def test_cpp_device_calls_match_python(built, tmp_path):
    """corner_subpix, a detect call with Handle::set_corner_subpix on, board_corners and Calibrator(recover) against the Python layer"""
    from chalkydri_amd import subpix
    from chalkydri_amd.detector import AprilTagDetector
    frames, fr, xy = _case(tmp_path)
    r = _run("device", SC.W, SC.H, 2, 5, tmp_path / "frames.bin", tmp_path / "points.bin", tmp_path / "out.bin")
    assert r.returncode == 0, (r.stdout, r.stderr)
    out, info = subpix.corner_subpix_host(frames, fr, xy, return_info=True)
    assert (tmp_path / "out.bin").read_bytes() == out.tobytes() + info.tobytes()
    det = AprilTagDetector(SC.W, SC.H, max_batch=2)
    for w in (0, 4):
        r = _run("detect", SC.W, SC.H, 2, w, tmp_path / "frames.bin", tmp_path / "dets.bin")
        assert r.returncode == 0, (r.stdout, r.stderr)
        det.set_corner_subpix(half_win=w or None, on=bool(w))
        want = det.detect_batch(frames)
        raw = (tmp_path / "dets.bin").read_bytes()
        counts = np.frombuffer(raw[:8], np.int32)
        assert counts.tolist() == [len(f) for f in want] and sum(counts) >= 6
        recs = np.frombuffer(raw[8:], np.dtype([("id", "<i4"), ("hamming", "<i4"), ("family", "<i4"), ("margin", "<f4"), ("c", "<f8", (2,)), ("p", "<f8", (4, 2))])).reshape(2, 64)
        for f in range(2):
            for k, d in enumerate(want[f]):
                assert recs[f, k]["id"] == d.id() and recs[f, k]["p"].tobytes() == d.corners().tobytes() and recs[f, k]["c"].tobytes() == d.center().tobytes()
    det.set_corner_subpix(on=False)
    r = _run("board", SC.W, SC.H, 2, 4, 4, tmp_path / "frames.bin", tmp_path / "board.bin")
    assert r.returncode == 0 and r.stdout.split()[:3] == ["OK", "2", "FRAMES"], (r.stdout, r.stderr)
    det.detect_batch(frames)
    uv, state = det.board_corners(SC.board())
    assert (state > 0).all()
    assert (tmp_path / "board.bin").read_bytes() == uv.tobytes() + state.tobytes() + np.array([16, 16], np.int32).tobytes()
    kept_recover, kept_plain = map(int, r.stdout.split()[3:5])
    assert kept_recover == 2 and kept_plain <= 2
    det.close()
