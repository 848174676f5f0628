"""The device solver of the mount calibration (k_rigcal.hip through ck_rigcal_refine_batch) against its bitwise
specification ck_rigcal_refine_host: mounts, poses, costs, per-camera rms, iterations and status compared as bytes.

Shapes, the smallest at which the mapping (16 lanes per view, 16 groups per workgroup, one thread per step's 6 x 6 solve) can still go
wrong: views of 1, 4, 5 and 17 tags (4, 16, 20, 68 points: one round of a lane group, exactly full, a second round, a fifth round);
2, 15, 16, 17 and 65 used steps of 2 cameras (30, 32 and 34 views: below, at and above two rounds of the 16 groups; 65 steps: more than
the 64 threads of a wave that factor one step each; 257 steps: a second round of the 256 threads that take one step each in the 6 x 6
solves, the step costs and the copy of accepted poses); 2, 3 and 8 cameras (8: the full 48 x 48 reduced system); a camera absent from
every other step; one-camera steps in the middle, which are skipped; all free / one position frozen / one camera wholly frozen besides
the gauge camera; max_iters = 3 (MAXIT).  Bearing noise 1e-3 everywhere, so that every solve takes several iterations."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

TAGS = (1, 4, 5, 17)
FIX0 = 0x3F
# name: (n_cams, n_steps, tags of (step, camera), fixed_mask, max_iters, min_steps)
CASES = {
    "tags_1_4_5_17": (2, 6, lambda s, c: TAGS[(s + c) % 4], FIX0, 100, 3),
    "steps2": (2, 2, lambda s, c: 2, FIX0, 100, 2),
    "steps15": (2, 15, lambda s, c: 1, FIX0, 100, 3),
    "steps16": (2, 16, lambda s, c: 1, FIX0, 100, 3),
    "steps17": (2, 17, lambda s, c: 1, FIX0, 100, 3),
    "steps65": (2, 65, lambda s, c: 1, FIX0, 100, 3),
    "steps257": (2, 257, lambda s, c: 1, FIX0, 100, 3),
    "cams3": (3, 6, lambda s, c: 2, FIX0, 100, 3),
    "cams8": (8, 5, lambda s, c: 1 + (s + c) % 2, FIX0, 100, 3),
    "absent": (3, 7, lambda s, c: 0 if (c == 2 and s % 2) else 2, FIX0, 100, 3),
    "skipped": (2, 8, lambda s, c: 0 if (c == 1 and s in (2, 3)) else 2, FIX0, 100, 3),
    "position_frozen": (3, 6, lambda s, c: 2, FIX0 | (0x38 << 6), 100, 3),
    "camera_frozen": (3, 6, lambda s, c: 2, FIX0 | (0x3F << 12), 100, 3),
    "maxit": (2, 6, lambda s, c: TAGS[(s + c) % 4], FIX0, 3, 3),
}


@pytest.fixture(scope="module")
def K(built):
    from chalkydri_amd import rigcal
    return rigcal


@pytest.fixture(scope="module")
def det(built):
    from chalkydri_amd.detector import AprilTagDetector
    d = AprilTagDetector(640, 480)      # the calls are not bound to the handle's geometry
    yield d
    d.close()


@pytest.fixture(scope="module")
def subsets(K):
    """A capture of 3 cameras x 12 steps and five half-subsets of it, each solved on the host once."""
    import rigcal_cases as RC
    case = RC.shape_case(7, 3, 12, lambda s, c: 1 + (s + c) % 3)
    rng = np.random.default_rng(11)
    probs = [sorted(rng.choice(12, 6, replace=False).tolist()) for _ in range(5)]
    p = K.params(FIX0)
    host = [K.refine_host(p, K.Capture(case["csteps"], [q]), case["m0"], case["poses0"]) for q in probs]
    return case, probs, p, host


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host(K, det, name):
    import rigcal_cases as RC
    n_cams, n_steps, n_tags, mask, max_iters, min_steps = CASES[name]
    case = RC.shape_case(3, n_cams, n_steps, n_tags)
    p = K.params(mask, max_iters=max_iters, min_steps=min_steps)
    cap = K.Capture(case["csteps"])
    want, wp = K.refine_host(p, cap, case["m0"], case["poses0"])
    res, poses = K.refine_batch(det, p, cap, case["m0"], case["poses0"])
    print(name, "status", int(want["status"]), "iters", int(want["iters"]), "rms", float(want["rms"]), "used", int(want["n_steps_used"]))
    assert res[0].tobytes() == want.tobytes(), (name, res[0], want)
    assert poses[0].tobytes() == wp.tobytes(), name
    if name == "maxit":
        assert want["status"] == A.CK_CALIB_MAXIT and want["iters"] == 3
    else:
        assert want["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED) and want["iters"] > 1 and want["cost"] < want["cost0"]
    if name == "skipped":
        assert want["n_steps"] == 8 and want["n_steps_used"] == 6
        assert wp[2:4].tobytes() == case["poses0"][2:4].tobytes()            # the skipped steps' poses come back as given
    if name == "camera_frozen":
        assert want["robot_to_cam"][2].tobytes() == bytes(case["m0"][2])
    if name == "position_frozen":
        o0, o1 = RC.mount_of(K, case["m0"][1])[1], RC.mount_of(K, want["robot_to_cam"][1])[1]
        assert np.abs(o0 - o1).max() < 1e-15 and not np.array_equal(want["robot_to_cam"][1]["q"], np.array(list(case["m0"][1].q)))


def test_batch_composition(K, det, subsets):
    """five subset problems in one call equal the five single calls, in two orders; a DEGENERATE problem in the middle (two steps:
    fewer than min_steps) leaves its neighbours' bytes alone"""
    case, probs, p, host = subsets
    for order in (list(range(5)), [4, 2, 0, 3, 1]):
        res, poses = K.refine_batch(det, p, K.Capture(case["csteps"], [probs[i] for i in order]), case["m0"], case["poses0"])
        for j, i in enumerate(order):
            assert _same((res[j], poses[j]), host[i]), (order, i)
    mixed = [probs[0], [3, 5], probs[1]]
    res, poses = K.refine_batch(det, p, K.Capture(case["csteps"], mixed), case["m0"], case["poses0"])
    assert _same((res[0], poses[0]), host[0]) and _same((res[2], poses[2]), host[1])
    deg = K.refine_host(p, K.Capture(case["csteps"], [[3, 5]]), case["m0"], case["poses0"])
    assert res[1]["status"] == A.CK_CALIB_DEGENERATE and _same((res[1], poses[1]), deg)
    assert poses[1].tobytes() == case["poses0"][[3, 5]].tobytes()
    assert all(res[1]["robot_to_cam"][c].tobytes() == bytes(case["m0"][c]) for c in range(3))


def test_problems_that_share_a_run(K, det, subsets):
    """two problems over the SAME run of step_index[] (the check allows it): refine_batch and calibrate_batch return both records equal
    to the single problem's, and the run's poses once"""
    case, probs, p, host = subsets
    one = K.Capture(case["csteps"], [probs[2]])
    two = K.Capture(case["csteps"], [probs[2]])
    two.prob = (A.RigcalProblem * 2)(one.prob[0], one.prob[0])
    two.n = 2
    res, poses = K.refine_batch(det, p, two, case["m0"], case["poses0"])
    assert len(res) == 2 and all(_same((res[i], poses[i]), host[2]) for i in range(2))
    gyro = np.zeros(12)
    want, wp = K.calibrate_batch(det, p, one, case["m0"], gyro)
    res, poses = K.calibrate_batch(det, p, two, case["m0"], gyro)
    assert all(res[i].tobytes() == want[0].tobytes() and poses[i].tobytes() == wp[0].tobytes() for i in range(2))
    full = K.Capture(case["csteps"])                                        # ... and every step of the capture, twice
    full2 = K.Capture(case["csteps"])
    full2.prob = (A.RigcalProblem * 2)(full.prob[0], full.prob[0])
    full2.n = 2
    want, wp = K.calibrate_batch(det, p, full, case["m0"], gyro)
    res, poses = K.calibrate_batch(det, p, full2, case["m0"], gyro)
    assert all(res[i].tobytes() == want[0].tobytes() and poses[i].tobytes() == wp[0].tobytes() for i in range(2))
    want, wp = K.refine_batch(det, p, full, case["m0"], case["poses0"])
    res, poses = K.refine_batch(det, p, full2, case["m0"], case["poses0"])
    assert all(res[i].tobytes() == want[0].tobytes() and poses[i].tobytes() == wp[0].tobytes() for i in range(2))


def test_two_runs_return_the_same_bytes(K, det, subsets):
    case, probs, p, host = subsets
    cap = K.Capture(case["csteps"], probs)
    a, b = K.refine_batch(det, p, cap, case["m0"], case["poses0"]), K.refine_batch(det, p, cap, case["m0"], case["poses0"])
    assert a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


def test_misuse_on_the_device(K, det, subsets):
    """refusals return their codes before the device is touched, and a valid call follows"""
    from chalkydri_amd import ChalkydriError
    case, probs, p, host = subsets
    cap = K.Capture(case["csteps"], [probs[0]])
    for bad, code in ((K.params(FIX0, max_iters=0), A.CK_EINVAL), (K.params(0), A.CK_EINVAL), (K.params(FIX0, min_cams_per_step=1), A.CK_EINVAL)):
        with pytest.raises(ChalkydriError) as e:
            K.refine_batch(det, bad, cap, case["m0"], case["poses0"])
        assert e.value.code == code
    past = K.Capture(case["csteps"], [probs[0]])
    past.step_index[len(probs[0]) - 1] = 12                                  # a step number past the capture
    with pytest.raises(ChalkydriError) as e:
        K.refine_batch(det, p, past, case["m0"], case["poses0"])
    assert e.value.code == A.CK_EINVAL
    res, poses = K.refine_batch(det, p, cap, case["m0"], case["poses0"])
    assert _same((res[0], poses[0]), host[0])


def test_mount_calibrator(K, det):
    """MountCalibrator end to end on a room capture of 3 cameras x 12 steps at bearing noise 1e-3, camera 1 and 2 off by up to 5 degrees
    and 5 cm: the calibrated mounts are nearer the truth than the starts, the rms is at the noise level, leave_out = 3 returns a
    finite spread."""
    import np_rigcal as N
    import rigcal_cases as RC
    rng = np.random.default_rng(5)
    mounts = N.make_mounts(rng, 3)
    steps, truth, gyro = N.make_capture(rng, mounts, 12, noise=1e-3)
    start = N.perturb_mounts(rng, mounts)
    mc = K.MountCalibrator(det=det, mounts0=[RC.mount_iso(m) for m in start])
    assert mc.add_steps(RC.c_steps(steps), gyro) == 12
    rep = mc.calibrate(leave_out=3)
    assert rep is not None and rep["status"] in ("converged", "stalled") and rep["rms"] < 3e-3
    for c in (1, 2):
        got = RC.mount_of(K, rep["robot_to_cam"][c])
        d0, d1 = N.mount_distance(start[c], mounts[c]), N.mount_distance(got, mounts[c])
        print("camera", c, "start", d0, "calibrated", d1)
        assert d1[0] < d0[0] and d1[1] < d0[1]
    assert rep["n_subsets"] >= 2 and all(np.isfinite(v) for c in range(3) for v in rep["std"][c].values())
    mc.clear()
    assert mc.observations() == [] and mc.calibrate() is None


# ---- with the detection pipeline ------------------------------------------------------------------------------------------------------
from test_gpu_rig import CAMS, rig_scene  # noqa: E402,F401  (the two rendered cameras of the rig tests and their four oracle-checked steps)

# camera 1 as the user typed it in: about 3 degrees and 3 cm off
WRONG1 = dict(CAMS[1][3], roll=1.5, pitch=-2.0, yaw=CAMS[1][3]["yaw"] + 1.5, x=CAMS[1][3]["x"] + 0.02, y=CAMS[1][3]["y"] - 0.02, z=CAMS[1][3]["z"] + 0.01)
# scipy trf against scipy lm on the observations of test_end_to_end_rendered, the larger of angle (rad) and position (m): 100 times it
# bounds the library's distance to trf.  Measured when the test was written: trf to lm 3.2e-12 rad / 4.86e-12 m (trf from a second start:
# 3.3e-12 / 2.8e-11); the library to trf 5.3e-11 rad / 1.7e-10 m
E2E_REFERENCE = 4.86e-12


def _tasks(r2c1, max_batch):
    import scenes
    from chalkydri_amd.apriltags import AprilTags
    layout = scenes.wall_layout(12)
    return [AprilTags(w, h, layout, scenes.pinhole_calib(f, w / 2.0, h / 2.0), r2c if c == 0 else r2c1, cam_id=c, max_batch=max_batch)
            for c, (w, h, f, r2c) in enumerate(CAMS)]


def test_last_pose_inputs(K, rig_scene):
    """after AprilTagsRig.process_batch the accessor returns, per camera, the known tags and corner bearings with which
    RigSolver.solve_batch reproduces last_results; the packed offsets; CK_ECAPACITY with the totals; CK_EINVAL after a plain detect"""
    import ctypes as C
    from chalkydri_amd import ChalkydriError
    from chalkydri_amd.rig import AprilTagsRig, RigSolver
    tasks, steps = rig_scene
    rig = AprilTagsRig(tasks, rig_id=42)
    gyro = [s["gyro"] for s in steps]
    frames = [np.stack([s["views"][c]["frame"] for s in steps]) for c in range(2)]
    rig.process_batch(frames, gyro)
    per_cam = [K.last_pose_inputs(t.detector, 4) for t in tasks]
    for c in range(2):
        at = 0
        for s, ((tags, bear), r) in enumerate(zip(*per_cam[c])):
            want_tags, want_bear, _ = steps[s]["views"][c]["input"]
            assert [bytes(t) for t in tags] == [bytes(t) for t in want_tags] and np.abs(bear - want_bear).max() < 1e-12
            assert (r.n_tags, r.n_bearings, r.tag_offset, r.bearing_offset) == (len(tags), 4 * len(tags), at, 4 * at)
            at += len(tags)
    again = RigSolver(tasks[0].detector, rig_id=42)
    again.params.sqpnp, again.params.sign_change_error = rig.solver.params.sqpnp, rig.solver.params.sign_change_error
    got = again.solve_batch([[per_cam[c][0][s] + (tasks[c].robot_to_cam,) for c in range(2)] for s in range(4)], gyro)
    assert got.tobytes() == rig.last_results.tobytes()
    # too small: the totals come back with CK_ECAPACITY
    L, rec, nt, nb = tasks[0].detector._L, (A.SqpnpProblem * 4)(), C.c_int32(0), C.c_int32(0)
    one, b = (A.Iso3 * 1)(), np.zeros((1, 3))
    assert L.ck_last_pose_inputs(tasks[0].detector._h, 4, rec, one, 0, b.ctypes.data, 0, C.byref(nt), C.byref(nb)) == A.CK_ECAPACITY
    assert nt.value == sum(len(t) for t, _ in per_cam[0][0]) and nb.value == 4 * nt.value
    assert L.ck_last_pose_inputs(tasks[0].detector._h, 3, rec, one, 0, b.ctypes.data, 0, C.byref(nt), C.byref(nb)) == A.CK_EINVAL
    tasks[1].detector.detect_batch(frames[1])
    with pytest.raises(ChalkydriError) as e:
        K.last_pose_inputs(tasks[1].detector, 4)
    assert e.value.code == A.CK_EINVAL


# ck_rig_calibrate_batch against the twin from the host rig solver's starts, measured when the test was written on this capture: 1.9e-15
# (the larger of angle in rad and position in m over the three mounts); the bound is 100 times that.  Propagated it is the same figure:
# the two rig solvers' starts differ by 4e-16 and the twin moves by 5.5 per unit of its starts there.
BOUND_CALIBRATE = 1.9e-13
BOUND_CALIBRATE_RMS = 2.2e-16       # the two rms differed by 2.2e-18


def test_calibrate_batch_against_the_twin(K, det):
    """ck_rig_calibrate_batch (starts from the rig solver on the device) against the twin from the host rig solver's starts on a room
    capture of 3 cameras x 12 steps at bearing noise 1e-3: the mounts within BOUND_CALIBRATE, the same used steps and iterations"""
    import rigcal_cases as RC
    import np_rigcal as N
    cs = RC.acceptance_case(3, 12, 2, 1e-3)
    p, cap = K.params(FIX0), K.Capture(cs["csteps"])
    gyro = [np.arctan2(R[0, 1], R[0, 0]) for R, _ in cs["truth"]]
    res, poses = K.calibrate_batch(det, p, cap, cs["m0"], gyro)
    want, _ = K.refine_host(p, K.Capture(cs["csteps"], [cs["ok"]]), cs["m0"], cs["poses0"])
    assert res[0]["status"] == want["status"] and res[0]["iters"] == want["iters"] and res[0]["n_steps_used"] == want["n_steps_used"]
    got = max(max(N.mount_distance(RC.mount_of(K, res[0]["robot_to_cam"][c]), RC.mount_of(K, want["robot_to_cam"][c]))) for c in range(3))
    print("calibrate_batch to twin:", got, "rms", float(res[0]["rms"]), float(want["rms"]))
    assert got <= BOUND_CALIBRATE and abs(res[0]["rms"] - want["rms"]) <= BOUND_CALIBRATE_RMS


def _e2e_scene():
    """16 instants of the two rendered cameras in front of the wall of 12 tags: 12 to calibrate on, 4 held out"""
    import scenes
    rng = np.random.default_rng(17)
    layout = scenes.wall_layout(12)
    poses = [(rng.uniform(1.2, 2.8), rng.uniform(-0.8, 0.8), rng.uniform(-0.3, 0.3)) for _ in range(16)]
    frames = [np.stack([scenes.render_view(5000 + 10 * i + c, w, h, f, layout, poses[i], r2c, noise_amp=1)[0] for i in range(16)])
              for c, (w, h, f, r2c) in enumerate(CAMS)]
    return poses, frames


def _fused_error(tasks, frames, poses):
    """mean position error (m) and heading error (rad) of the rig's fused pose over the instants that gave one"""
    from chalkydri_amd.rig import AprilTagsRig
    recs, valid, _ = AprilTagsRig(tasks).process_batch(frames, [p[2] for p in poses])
    err = [(np.hypot(r.pose_x - p[0], r.pose_y - p[1]), abs((r.pose_rot - p[2] + np.pi) % (2 * np.pi) - np.pi)) for r, v, p in zip(recs, valid, poses) if v]
    assert len(err) >= 3
    return np.mean(err, 0)


def e2e_measure(K):
    """the observations and the library's and scipy's solves of the end-to-end test (also run by itself to measure E2E_REFERENCE)"""
    import np_rigcal as N
    import rigcal_cases as RC
    from chalkydri_amd.rig import AprilTagsRig, RigSolver
    poses, frames = _e2e_scene()
    tasks = _tasks(WRONG1, 16)
    mc = K.MountCalibrator(AprilTagsRig(tasks))
    mc.process([f[:12] for f in frames], [p[2] for p in poses[:12]])
    obs = mc.observations()
    rep = mc.calibrate(leave_out=3)
    # scipy on the same observations from the same kind of start (the host rig solver's poses with the wrong mount)
    steps = [[([(N.quat_to_mat(list(t.q)), np.array(list(t.t))) for t in tg], b) for tg, b in cams] for cams in obs]
    m0 = [RC.mount_of(K, m) for m in mc.mounts0]
    solver = RigSolver()
    solver.params.sign_change_error = 0.0
    rr = solver.solve_host([[(tg, b, m) for (tg, b), m in zip(cams, mc.mounts0)] for cams in obs], [p[2] for p in poses[:12]])
    ok = [s for s in range(12) if rr[s]["valid"]]
    prob = N.Problem([steps[s] for s in ok], 2)
    p0 = [(K.start_poses(rr)[ok[u], :9].reshape(3, 3), K.start_poses(rr)[ok[u], 9:]) for u in prob.used]
    free = [[False] * 6, [True] * 6]
    trf = N.solve(prob, m0, p0, free)[0]
    return {"tasks": tasks, "poses": poses, "frames": frames, "rep": rep, "prob": prob, "m0": m0, "p0": p0, "free": free, "trf": trf, "mc": mc}


def test_end_to_end_rendered(K):
    """Two rendered cameras, 12 instants, camera 1's mount typed in 3 degrees and 3 cm off: MountCalibrator.process then calibrate.
    The calibrated mount against scipy trf's on the same observations: bound 100 times trf against lm there (E2E_REFERENCE); the fused
    pose of AprilTagsRig on 4 held-out instants is nearer the truth with the calibrated mount than with the wrong one; the returned
    offsets are what AprilTags(..., robot_to_cam=) takes; leave_out = 3 returns a finite spread."""
    import np_rigcal as N
    import rigcal_cases as RC
    m = e2e_measure(K)
    rep = m["rep"]
    assert rep is not None and rep["status"] in ("converged", "stalled") and rep["n_steps_used"] >= 8
    got = RC.mount_of(K, rep["robot_to_cam"][1])
    d = max(N.mount_distance(got, m["trf"][1]))
    true1 = RC.mount_of(K, _tasks(CAMS[1][3], 1)[1].robot_to_cam)
    print("to scipy", d, "start to the truth", N.mount_distance(m["m0"][1], true1), "calibrated to the truth", N.mount_distance(got, true1), "rms", rep["rms"],
          "spread", rep["std"][1] if rep["std"] else None)
    assert d <= 100 * E2E_REFERENCE
    assert rep["n_subsets"] >= 2 and all(np.isfinite(v) for v in rep["std"][1].values())
    held = [f[12:] for f in m["frames"]]
    wrong = _fused_error(m["tasks"], held, m["poses"][12:])
    fixed = _fused_error(_tasks(rep["offsets"][1], 16), held, m["poses"][12:])
    print("held-out fused pose error (m, rad): wrong mount", wrong, "calibrated", fixed)
    assert fixed[0] < wrong[0]
