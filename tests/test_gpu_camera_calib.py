"""The EUCM / UCM calibration on the MI355X (ck_camera_calib_refine_batch, ck_camera_calibrate_batch, k_calib_eucm.hip):
every byte of the device's results and poses equals the host twin's at the shapes where the kernel's walkers can go wrong; the
multi-start call returns what six host solves and the same selection rule return; OpenCVModel5 through the new entry point is the old
one; Calibrator.calibrate(model="EUCM") end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_calib as N  # noqa: E402
import np_camera as NC  # noqa: E402
import np_camera_calib as M  # noqa: E402
from test_camera_calib_host import parallel_frames, solve_all_starts  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = (3, 4, 5)                      # per problem: one more than the workgroup's four waves
POINTS = (24, 63, 64, 65, 130)          # per frame: around the lane stride of 64, and more than two rounds of it


@pytest.fixture(scope="module")
def K(built):
    from chalkydri_amd import calibration
    return calibration


@pytest.fixture(scope="module")
def det(built):
    from chalkydri_amd.detector import AprilTagDetector
    d = AprilTagDetector(NC.W, NC.H)
    yield d
    d.close()


def _frames_with(lens, F, npts, seed):
    """F frames of exactly npts points each, spread over the board."""
    frames, _ = M.make_case(lens, F, 0.1, seed, min_points=npts)
    out = []
    for b, u in frames:
        idx = np.round(np.linspace(0, len(b) - 1, npts)).astype(int)
        out.append((b[idx], u[idx]))
    return out


@pytest.fixture(scope="module")
def shapes():
    """Per lens the 15 problems F x points, made once and shared."""
    return {name: [_frames_with(NC.LENSES[name], F, n, 10 * F + n) for F in FRAMES for n in POINTS] for name in ("eucm_wide", "ucm")}


def _same(res_d, poses_d, res_h, poses_h, what):
    assert res_d.tobytes() == res_h.tobytes(), (what, res_d, res_h)
    assert poses_d.tobytes() == poses_h.tobytes(), what


@pytest.mark.parametrize("mask,max_iters", [(0, 100), (1 << 5, 100), (0x003, 100), (0, 1)])
@pytest.mark.parametrize("name", ["eucm_wide", "ucm"])
def test_device_equals_host_bytes(K, det, shapes, name, mask, max_iters):
    """One batch of the 15 shapes and one problem without a usable start (a zero camera) in its middle, against 15 host solves: results
    and poses byte for byte.  fixed_mask: none, beta frozen, fx fy frozen; one iteration and a hundred.  Two problems again alone:
    a problem's result does not depend on its neighbours.  The batch twice: the same bytes."""
    model = "UCM" if name == "ucm" else "EUCM"
    p = K.params(NC.W, NC.H, fixed_mask=mask, max_iters=max_iters)
    problems = list(shapes[name])
    starts = [K.camera_calib_init(model, p, fr, 2)[:2] for fr in problems]         # the 0.45 max(w, h) start
    problems.insert(7, problems[3])
    starts.insert(7, (np.zeros(9), starts[3][1]))                                   # fx = 0: DEGENERATE
    res, poses = K.camera_refine_batch(det, model, p, problems, [s[0] for s in starts], [s[1] for s in starts])
    statuses = set()
    for i, (fr, (k0, p0)) in enumerate(zip(problems, starts)):
        rh, ph = K.camera_refine_host(model, p, fr, k0, p0)
        _same(res[i], poses[i], rh, ph, (i, len(fr), len(fr[0][0])))
        statuses.add(int(rh["status"]))
    assert res[7]["status"] == A.CK_CALIB_DEGENERATE and res[7]["iters"] == 0 and poses[7].tobytes() == starts[7][1].tobytes()
    assert statuses - {A.CK_CALIB_DEGENERATE} and (max_iters > 1 or statuses == {A.CK_CALIB_MAXIT, A.CK_CALIB_DEGENERATE})
    if max_iters > 1:
        assert A.CK_CALIB_CONVERGED in statuses or A.CK_CALIB_STALLED in statuses
        print(name, mask, "status:rms", ["%d:%.3g" % (r["status"], r["rms"]) for r in res])
    for i in (0, 14):
        r1, p1 = K.camera_refine_batch(det, model, p, [problems[i]], [starts[i][0]], [starts[i][1]])
        _same(r1[0], p1[0], res[i], poses[i], ("solo", i))
    res2, poses2 = K.camera_refine_batch(det, model, p, problems, [s[0] for s in starts], [s[1] for s in starts])
    assert res2.tobytes() == res.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(poses, poses2))


def test_opencv5_through_the_camera_entry_point_is_the_old_one(K, det):
    k, w, h = N.cameras()["cam1_1600x1304"]
    problems = [N.make_case(k, w, h, F, 0.1, F)[0] for F in (3, 5, 4)]
    for mask in (0, A.CK_CALIB_FIX_DISTORTION):
        p = K.params(w, h, fixed_mask=mask)
        starts = [K.calib_init(p, fr)[:2] for fr in problems]
        res, poses = K.refine_batch(det, p, problems, [s[0] for s in starts], [s[1] for s in starts])
        resc, posesc = K.camera_refine_batch(det, "OpenCVModel5", p, problems, [s[0] for s in starts], [s[1] for s in starts])
        for f in ("cam", "status", "iters", "n_frames", "n_points", "rms", "cost0", "cost"):
            assert resc[f].tobytes() == res[f].tobytes(), f
        assert all(a.tobytes() == b.tobytes() for a, b in zip(poses, posesc)) and (res["status"] != A.CK_CALIB_DEGENERATE).all()
        res, poses = K.calibrate_batch(det, p, problems)
        resc, posesc = K.camera_calibrate_batch(det, "OpenCVModel5", p, problems)
        for f in ("cam", "status", "iters", "n_frames", "n_points", "rms", "cost0", "cost"):
            assert resc[f].tobytes() == res[f].tobytes(), f
        assert all(a.tobytes() == b.tobytes() for a, b in zip(poses, posesc)) and (resc["n_starts"] == 1).all() and not resc["start"].any()


def test_multi_start_returns_the_minimum_cost_start(K, det):
    """ck_camera_calibrate_batch = ck_camera_calib_init + ck_camera_calib_refine_host for s = 0..5 on the host and the same rule (lowest
    finite final cost, lowest index on ties): the record, `start`, `n_starts` and the poses, byte for byte.  One 8-frame capture of the
    wide lens at 0.1 px; a capture of frames parallel to the image plane in the same call is DEGENERATE and disturbs nobody."""
    lens = NC.LENSES["eucm_wide"]
    p = K.params(NC.W, NC.H)
    cap8, _ = M.make_case(lens, 8, 0.1, 0)
    cap4, _ = M.make_case(lens, 4, 0.1, 1)          # (on the host: start 0 of this one has no focal length, start 5 ends far away)
    flat = parallel_frames(4, 0)
    res, poses = K.camera_calibrate_batch(det, "EUCM", p, [cap8, flat, cap4])
    for i, cap in ((0, cap8), (2, cap4)):
        win, outs = solve_all_starts(K, "EUCM", p, cap)
        want = outs[win][0].copy()
        want["start"], want["n_starts"] = win, A.CK_CAMCAL_STARTS
        _same(res[i], poses[i], want, outs[win][1], i)
        assert res[i]["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED) and res[i]["rms"] < 0.16
        assert np.abs(res[i]["cam"][:6] - lens).max() < 1.0
        print("capture", i, "winner", win, "finals", ["%d:%.3g" % (o[0]["status"], o[0]["rms"]) for o in outs])
    assert res[1]["status"] == A.CK_CALIB_DEGENERATE and res[1]["n_starts"] == A.CK_CAMCAL_STARTS and res[1]["start"] == 0
    assert not poses[1].any() and res[1]["iters"] == 0
    ru, pu = K.camera_calibrate_batch(det, "UCM", p, [cap8])
    win, outs = solve_all_starts(K, "UCM", p, cap8)
    want = outs[win][0].copy()
    want["start"], want["n_starts"] = win, A.CK_CAMCAL_STARTS
    _same(ru[0], pu[0], want, outs[win][1], "ucm")


def test_calibrator_eucm_end_to_end(K, built):
    """Calibrator.calibrate(model="EUCM") from board correspondences synthesised with the restatement (8 frames, 0.1 px): the blob is
    the lens, loads into AprilTags(calib=), and the leave_out = 4 spreads are finite."""
    import scenes
    from chalkydri_amd import Calibrator
    from chalkydri_amd.apriltags import AprilTags
    from chalkydri_amd.detector import AprilTagDetector
    lens = NC.LENSES["eucm_wide"]
    d = AprilTagDetector(NC.W, NC.H)
    cal = Calibrator(d)
    for b, u in M.make_case(lens, 8, 0.1, 3)[0]:
        assert cal.add_observations(b, u)
    assert not cal.add_observations(b[:5], u[:5]) and len(cal.observations()) == 8
    calib, report = cal.calibrate(model="EUCM", leave_out=4)
    d.close()
    m = calib["EUCM"]
    assert set(m) == {"fx", "fy", "cx", "cy", "alpha", "beta", "width", "height"} and (m["width"], m["height"]) == (NC.W, NC.H)
    got = np.array([m[f] for f in ("fx", "fy", "cx", "cy", "alpha", "beta")])
    print("EUCM from 8 frames at 0.1 px:", got, "rms", report["rms"], "start", report["start"], "std", report["std"])
    assert report["status"] in ("converged", "stalled") and report["rms"] < 0.16 and max(report["per_frame_rms"]) < 0.2
    assert np.abs(got - lens).max() < 1.0 and abs(got[4] - lens[4]) < 0.01 and abs(got[5] - lens[5]) < 0.02
    assert report["n_starts"] == A.CK_CAMCAL_STARTS and report["n_subsets"] >= 2
    assert set(report["std"]) == {"fx", "fy", "cx", "cy", "alpha", "beta"} and all(np.isfinite(v) for v in report["std"].values())
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
    task = AprilTags(NC.W, NC.H, scenes.wall_layout(6, cols=3), calib, r2c)
    assert task.camera.model == A.CK_CAMERA_EUCM and list(task.camera.k[:6]) == list(got) and task.detector.camera is task.camera
    task.detector.close()
    u = Calibrator(AprilTagDetector(NC.W, NC.H))
    for b, uv in M.make_case(NC.LENSES["ucm"], 4, 0.1, 1)[0]:
        u.add_observations(b, uv)
    calib, report = u.calibrate(model="UCM")
    u.det.close()
    assert set(calib["UCM"]) == {"fx", "fy", "cx", "cy", "alpha", "width", "height"} and abs(calib["UCM"]["alpha"] - 0.55) < 0.01
