"""The device solver of the field calibration (k_fieldcal.hip through ck_fieldcal_refine_batch) against its bitwise
specification ck_fieldcal_refine_host: results, layouts, per-tag sightings and rms and poses compared as bytes.

Shapes, the smallest at which the mapping (4 lanes per sighting, 64 groups per workgroup, one thread per pair and per step, one
thread per entry of the reduced system, rows t and t + 256 of its factorisation) can still go wrong: 2 (one free), 3, 10 and 11 tags
with sightings (60 and 66 unknowns, either side of a wave), 42 and 43 (252 and 258, either side of the 256 threads that own the rows),
64 (the cap, 384); 2, 255, 256 and 257 used steps; 2, 3 and 17 tags per step; a tag seen by two and by three cameras in one step; a
camera absent from every other step; one-tag steps in the middle, which are skipped; a layout entry never seen; partial masks;
max_iters = 3 (MAXIT).  Bearing noise 1e-3 everywhere, so that every solve takes several iterations."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

DONE = (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED)


def _ring(n_tags, per_step, stride=1):
    return lambda s, c: [(s * stride + c + j) % n_tags for j in range(per_step)]


# name: (n_cams, n_steps, n_layout, tags of (step, camera), masks or None (tag 0 the gauge), max_iters, min_steps)
CASES = {
    "tags2": (1, 4, 2, lambda s, c: [0, 1], None, 100, 3),
    "tags3": (1, 5, 3, _ring(3, 2), None, 100, 3),
    "tags10": (2, 12, 10, _ring(10, 3), None, 100, 3),
    "tags11": (2, 12, 11, _ring(11, 3), None, 100, 3),
    "tags42": (2, 24, 42, _ring(42, 3, 2), None, 100, 3),
    "tags43": (2, 24, 43, _ring(43, 3, 2), None, 100, 3),
    "tags64": (2, 44, 64, _ring(64, 6, 3), None, 100, 3),
    "steps2": (1, 2, 3, lambda s, c: [0, 1, 2], None, 100, 2),
    "steps255": (1, 255, 6, _ring(6, 2), None, 100, 3),
    "steps256": (1, 256, 6, _ring(6, 2), None, 100, 3),
    "steps257": (1, 257, 6, _ring(6, 2), None, 100, 3),
    "per_step3": (1, 8, 7, _ring(7, 3), None, 100, 3),
    "per_step17": (1, 5, 20, _ring(20, 17, 4), None, 100, 3),
    "cams2_cams3": (3, 10, 5, lambda s, c: [s % 5] if c == 2 else [(s + j) % 5 for j in range(3 - c)], None, 100, 3),
    "absent": (3, 8, 6, lambda s, c: [] if (c == 2 and s % 2) else [(s + c + j) % 6 for j in range(2)], None, 100, 3),
    "skipped": (2, 9, 5, lambda s, c: [s % 5] if s in (3, 4) else [(s + c + j) % 5 for j in range(2)], None, 100, 3),
    "unseen": (2, 7, 6, _ring(5, 2), None, 100, 3),
    "masks": (2, 8, 5, _ring(5, 3), {0: 63, 1: 0x38, 2: 0x07, 3: 0b010010}, 100, 3),
    "maxit": (2, 8, 5, _ring(5, 3), None, 3, 3),
}


@pytest.fixture(scope="module")
def K(built):
    from chalkydri_amd import fieldcal
    return fieldcal


@pytest.fixture(scope="module")
def det(built):
    from chalkydri_amd.detector import AprilTagDetector
    d = AprilTagDetector(640, 480)      # the calls are not bound to the handle's geometry
    yield d
    d.close()


def _args(case):
    return case["m_iso"], case["lay0"], case["fixed"], case["poses0"]


@pytest.fixture(scope="module")
def subsets(K):
    """A capture of 3 cameras x 12 steps over 8 tags and five half-subsets of it, each solved on the host once."""
    import fieldcal_cases as FC
    case = FC.shape_case(7, 3, 12, 8, lambda s, c: [(s + 2 * c + j) % 8 for j in range(1 + (s + c) % 3)])
    rng = np.random.default_rng(11)
    probs = [sorted(rng.choice(12, 6, replace=False).tolist()) for _ in range(5)]
    p = K.params()
    host = [K.refine_host(p, K.Capture(case["steps"], [q]), *_args(case)) for q in probs]
    return case, probs, p, host


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _pick(out, i):
    return tuple(o[i] for o in out)


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host(K, det, name):
    import fieldcal_cases as FC
    n_cams, n_steps, n_layout, seen, masks, max_iters, min_steps = CASES[name]
    case = FC.shape_case(3, n_cams, n_steps, n_layout, seen, masks=masks)
    p = K.params(max_iters=max_iters, min_steps=min_steps)
    cap = K.Capture(case["steps"])
    want = K.refine_host(p, cap, *_args(case))
    got = _pick(K.refine_batch(det, p, cap, *_args(case)), 0)
    res, lay, sight, rms, poses = want
    print(name, "status", int(res["status"]), "iters", int(res["iters"]), "rms", float(res["rms"]), "used", int(res["n_steps_used"]), "tags",
          int(np.sum(sight > 0)), "solved", int(res["n_tags_solved"]))
    for what, a, b in zip(("result", "layout", "sightings", "tag rms", "poses"), got, want):
        assert a.tobytes() == b.tobytes(), (name, what, a, b)
    if name == "maxit":
        assert res["status"] == A.CK_CALIB_MAXIT and res["iters"] == 3
    else:
        assert res["status"] in DONE and res["iters"] > 1 and res["cost"] < res["cost0"]
    assert lay[0].tobytes() == bytes(case["lay0"][0])
    if name.startswith("tags"):
        assert np.sum(sight > 0) == int(name[4:]) and res["n_tags_solved"] == int(name[4:]) - 1
    if name == "skipped":
        assert res["n_steps"] == 9 and res["n_steps_used"] == 7
        assert poses[3:5].tobytes() == case["poses0"][3:5].tobytes()           # the skipped steps' poses come back as given
    if name == "unseen":
        assert sight[5] == 0 and rms[5] == 0 and lay[5].tobytes() == bytes(case["lay0"][5])
    if name == "masks":
        raw = lambda k: np.frombuffer(bytes(case["lay0"][k]), np.float64)
        assert np.array_equal(lay[1]["t"], raw(1)[:3]) and not np.array_equal(lay[1]["q"], raw(1)[3:])
        assert np.array_equal(lay[2]["q"], raw(2)[3:]) and not np.array_equal(lay[2]["t"], raw(2)[:3])
        assert lay[3]["t"][1] == raw(3)[1] and lay[3]["t"][0] != raw(3)[0] and lay[3]["t"][2] != raw(3)[2]


def test_batch_composition(K, det, subsets):
    """five subset problems in one call equal the five single calls, in two orders; a DEGENERATE problem in the middle (two steps:
    fewer than min_steps) leaves its neighbours' bytes alone"""
    case, probs, p, host = subsets
    for order in (list(range(5)), [4, 2, 0, 3, 1]):
        out = K.refine_batch(det, p, K.Capture(case["steps"], [probs[i] for i in order]), *_args(case))
        for j, i in enumerate(order):
            assert _same(_pick(out, j), host[i]), (order, i)
    mixed = [probs[0], [3, 5], probs[1]]
    out = K.refine_batch(det, p, K.Capture(case["steps"], mixed), *_args(case))
    assert _same(_pick(out, 0), host[0]) and _same(_pick(out, 2), host[1])
    deg = K.refine_host(p, K.Capture(case["steps"], [[3, 5]]), *_args(case))
    assert out[0][1]["status"] == A.CK_CALIB_DEGENERATE and _same(_pick(out, 1), deg)
    assert out[4][1].tobytes() == case["poses0"][[3, 5]].tobytes()
    assert out[1][1].tobytes() == b"".join(bytes(t) for t in case["lay0"]) and not out[3][1].any()


def test_two_runs_return_the_same_bytes(K, det, subsets):
    case, probs, p, host = subsets
    cap = K.Capture(case["steps"], probs)
    a, b = K.refine_batch(det, p, cap, *_args(case)), K.refine_batch(det, p, cap, *_args(case))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4])) and all(x.tobytes() == y.tobytes() for x, y in zip(a[4], b[4]))


def test_misuse_on_the_device(K, det, subsets):
    """refusals return their codes before the device is touched, and a valid call follows"""
    from chalkydri_amd import ChalkydriError
    case, probs, p, host = subsets
    cap = K.Capture(case["steps"], [probs[0]])
    m, lay, fx, p0 = _args(case)
    dup = K.Capture(case["steps"], [probs[0]])
    r = next(r for r in dup.records if r.n_tags >= 2)
    dup.tag_index[r.tag_offset + 1] = dup.tag_index[r.tag_offset]
    past = K.Capture(case["steps"], [probs[0]])
    past.step_index[len(probs[0]) - 1] = 12                                  # a step number past the capture
    for bad_p, bad_cap, bad_fx in ((K.params(max_iters=0), cap, fx), (K.params(min_tags_per_step=1), cap, fx), (p, cap, np.zeros(8, np.uint8)),
                                   (p, dup, fx), (p, past, fx)):
        with pytest.raises(ChalkydriError) as e:
            K.refine_batch(det, bad_p, bad_cap, m, lay, bad_fx, p0)
        assert e.value.code == A.CK_EINVAL
        with pytest.raises(ChalkydriError) as e:
            K.calibrate_batch(det, bad_p, bad_cap, m, lay, bad_fx, np.zeros(12))
        assert e.value.code == A.CK_EINVAL
    assert _same(_pick(K.refine_batch(det, p, cap, *_args(case)), 0), host[0])


# ck_field_calibrate_batch against the twin from the host rig solver's starts, measured when the test was written on this capture (the
# largest angle in rad or distance in m over the tags with sightings); the bound is 100 times that.
MEASURED_CALIBRATE = 1.99e-14
BOUND_CALIBRATE = 100 * MEASURED_CALIBRATE
BOUND_CALIBRATE_RMS = 1e-9          # relative


def test_calibrate_batch_against_the_twin(K, det):
    """ck_field_calibrate_batch (starts from the rig solver on the device) against the twin from the host rig solver's starts on a room
    capture of 3 cameras x 40 steps at bearing noise 1e-3: the layout within BOUND_CALIBRATE, the same used steps and iterations"""
    import fieldcal_cases as FC
    import np_fieldcal as N
    cs = FC.acceptance_case(3, 40, 0, 1e-3)
    p, cap = K.params(), K.Capture(cs["steps"])
    res, lay, sight, rms, poses = K.calibrate_batch(det, p, cap, cs["m_iso"], cs["lay0"], cs["fixed"], cs["gyro"])
    want, wlay, wsight, wrms, _ = K.refine_host(p, K.Capture(cs["steps"], [cs["ok"]]), cs["m_iso"], cs["lay0"], cs["fixed"], cs["poses0"])
    assert res[0]["status"] == want["status"] and res[0]["iters"] == want["iters"] and res[0]["n_steps_used"] == want["n_steps_used"]
    assert sight[0].tobytes() == wsight.tobytes()
    seen = [k for k in range(len(wsight)) if wsight[k] > 0]
    got = N.layout_distance(FC.layout_of(lay[0]), FC.layout_of(wlay), seen)
    print("calibrate_batch to twin:", got, "rms", float(res[0]["rms"]), float(want["rms"]), "bound", BOUND_CALIBRATE)
    assert got <= BOUND_CALIBRATE and abs(res[0]["rms"] - want["rms"]) <= BOUND_CALIBRATE_RMS * want["rms"]


def test_field_calibrator(K, det):
    """FieldCalibrator through add_steps on a room capture of one camera x 60 steps at bearing noise 1e-3: the default gauge is the tag
    with the most sightings; the layout equals calibrate_batch's; the moved distances, the spread of leave_out = 3 and the field.json
    dict are there and load as a layout; two layout entries with the same pose are refused"""
    import fieldcal_cases as FC
    from chalkydri_amd.apriltags import load_field_layout
    cs = FC.acceptance_case(1, 60, 0, 1e-3)
    ids = [100 + 3 * k for k in range(len(cs["lay0"]))]
    nominal = K.layout_dict(ids, cs["lay0"], {"length": 8.0, "width": 6.0})
    fc = K.FieldCalibrator(det=det, mounts=cs["m_iso"], layout=nominal)
    assert fc.add_steps([[([ids[k] for k in tg], b) for tg, b in cams] for cams in cs["steps"]], cs["gyro"]) == 60
    assert int(np.argmax(fc.fixed6())) == cs["gauge"] and fc.fixed6()[cs["gauge"]] == 63 and np.sum(fc.fixed6() > 0) == 1
    rep = fc.calibrate(leave_out=3)
    assert rep is not None and rep["status"] in ("converged", "stalled") and rep["rms"] < 3e-3 and rep["layout"]["field"] == nominal["field"]
    back = load_field_layout(rep["layout"])
    res, lay, sight, rms, _ = K.calibrate_batch(det, K.params(), K.Capture(cs["steps"]), cs["m_iso"], fc.layout0, cs["fixed"], cs["gyro"])
    assert sorted(back) == ids and all(np.allclose(list(back[ids[k]].t), lay[0][k]["t"], atol=1e-15) for k in range(len(ids)))
    seen = [k for k in range(len(ids)) if sight[0][k] > 0]
    assert all(rep["tags"][ids[k]]["sightings"] == sight[0][k] and rep["tags"][ids[k]]["rms"] == rms[0][k] for k in range(len(ids)))
    assert rep["tags"][ids[cs["gauge"]]]["moved"] == (0.0, 0.0) and sum(rep["tags"][ids[k]]["moved"][0] > 1e-3 for k in seen) >= len(seen) - 3
    assert rep["n_subsets"] >= 2 and any(rep["tags"][ids[k]]["std"] is not None and np.all(np.isfinite(rep["tags"][ids[k]]["std"])) for k in seen)
    assert [[list(i) for i, _ in cams] for cams in fc.observations()] == [[[ids[k] for k in tg] for tg, _ in cams] for cams in cs["steps"]]
    fc.clear()
    assert fc.observations() == [] and fc.calibrate() is None
    twice = dict(nominal, tags=nominal["tags"] + [dict(nominal["tags"][0], ID=999)])
    with pytest.raises(ValueError):
        K.FieldCalibrator(det=det, mounts=cs["m_iso"], layout=twice)


# ---- with the detection pipeline ------------------------------------------------------------------------------------------------------
from test_gpu_rig import CAMS  # noqa: E402  (the two rendered cameras of the rig tests)

MOVED = (3, 8, 10)                     # ids of the tags rendered 2 cm and 1.5 degrees (about their normal) away from the drawing

def _rendered_layout():
    """the wall of 12 tags as drawn, and as built: three tags moved"""
    import copy
    import scenes
    nominal = scenes.wall_layout(12)
    built_ = copy.deepcopy(nominal)
    rng = np.random.default_rng(23)
    for t in built_["tags"]:
        if t["ID"] in MOVED:
            d = rng.normal(size=3)
            d *= 0.02 / np.linalg.norm(d)
            for k, a in enumerate("xyz"):
                t["pose"]["translation"][a] += float(d[k])
            q = t["pose"]["rotation"]["quaternion"]
            w, x, y, z = q["W"], q["X"], q["Y"], q["Z"]                      # q * (cos, sin, 0, 0): a turn about the tag's own x
            c, s = np.cos(np.radians(0.75)), np.sin(np.radians(0.75)) * (1 if t["ID"] % 2 else -1)
            q["W"], q["X"], q["Y"], q["Z"] = float(w * c - x * s), float(w * s + x * c), float(y * c + z * s), float(z * c - y * s)
    return nominal, built_


def _e2e_tasks(layout, max_batch):
    import scenes
    from chalkydri_amd.apriltags import AprilTags
    return [AprilTags(w, h, layout, scenes.pinhole_calib(f, w / 2.0, h / 2.0), r2c, cam_id=c, max_batch=max_batch) for c, (w, h, f, r2c) in enumerate(CAMS)]


def _e2e_scene():
    """16 instants of the two rendered cameras in front of the wall as built: 12 to calibrate on, 4 held out"""
    import scenes
    rng = np.random.default_rng(17)
    built_ = _rendered_layout()[1]
    poses = [(rng.uniform(1.2, 2.8), rng.uniform(-0.8, 0.8), rng.uniform(-0.3, 0.3)) for _ in range(16)]
    frames = [np.stack([scenes.render_view(5000 + 10 * i + c, w, h, f, built_, poses[i], r2c, noise_amp=1)[0] for i in range(16)])
              for c, (w, h, f, r2c) in enumerate(CAMS)]
    return poses, frames


def _corner_distance(a, b):
    """rms distance (m) of the four corners of two tag poses.  A tag enters every solver through its four corners only, so this is how
    far one pose is from another for the pipeline; a turn about an axis in the tag's plane by `a` rad moves the corners by at most
    0.117 a, which is why that part of a single tag's rotation stays at the noise level at a dozen sightings (the report's own
    leave-out spread says so) while its position and its corners are resolved to millimetres."""
    import np_fieldcal as N
    from chalkydri_amd.rigcal import iso_matrix
    (Ra, ta), (Rb, tb) = iso_matrix(a), iso_matrix(b)
    return float(np.sqrt(np.mean(np.sum(((N.CORNERS @ Ra.T + ta) - (N.CORNERS @ Rb.T + tb)) ** 2, 1))))


def _collect(K, frames, poses, max_batch=16):
    from chalkydri_amd.rig import AprilTagsRig
    tasks = _e2e_tasks(_rendered_layout()[0], max_batch)
    fc = K.FieldCalibrator(AprilTagsRig(tasks), layout=_rendered_layout()[0])
    fc.process([f[:12] for f in frames], [p[2] for p in poses[:12]])
    return tasks, fc


def _fused_error(tasks, frames, poses):
    """mean position error (m) and heading error (rad) of the rig's fused pose over the instants that gave one"""
    from chalkydri_amd.rig import AprilTagsRig
    recs, valid, _ = AprilTagsRig(tasks).process_batch(frames, [p[2] for p in poses])
    err = [(np.hypot(r.pose_x - p[0], r.pose_y - p[1]), abs((r.pose_rot - p[2] + np.pi) % (2 * np.pi) - np.pi)) for r, v, p in zip(recs, valid, poses) if v]
    assert len(err) >= 3
    return np.mean(err, 0)


def test_end_to_end_rendered(K):
    """Two rendered cameras, 12 instants in front of a wall of 12 tags of which three hang 2 cm and 1.5 degrees away from the layout
    the detector is given: FieldCalibrator.process (ids matched through the pose bytes of ck_last_pose_inputs), then calibrate.
    The moved tags come back nearer where they were rendered than the
    drawing has them, in position and in the distance of their corners (measured when the test was written: positions 20 mm -> 1.7,
    6.0 and 1.5 mm; the total rotation angle, 0.026 rad in the drawing, stays at the noise of a single 16 cm tag, 0.032, 0.006 and 0.029
    rad, with a leave-out spread of 0.010 .. 0.023 rad: see _corner_distance); the layout against scipy trf's on the same observations within 100 times trf against lm there (both solved here); the fused pose
    of AprilTagsRig on 4 held-out instants is nearer the truth with the calibrated layout than with the nominal one."""
    import fieldcal_cases as FC
    import np_fieldcal as N
    from chalkydri_amd import rigcal
    from chalkydri_amd.apriltags import load_field_layout
    from chalkydri_amd.rig import RigSolver
    nominal, built_ = _rendered_layout()
    poses, frames = _e2e_scene()
    tasks, fc = _collect(K, frames, poses)
    obs = fc.observations()
    count = {}
    for cams in obs:
        for ids, _ in cams:
            for i in ids:
                count[i] = count.get(i, 0) + 1
    assert all(i in count for i in MOVED) and len(count) >= 8
    # four surveyed tags stay where the drawing has them: a single gauge tag on a single wall pins the gauge by its own 16 cm only, and
    # the whole wall then pivots about it with the noise ("Rendered end to end")
    frozen = sorted((i for i in count if i not in MOVED), key=lambda i: -count[i])[:4]
    rep = fc.calibrate(fixed={i: K.FIX_ALL for i in frozen}, leave_out=3)
    assert rep is not None and rep["status"] in ("converged", "stalled") and rep["n_steps_used"] >= 8
    # the moved tags
    nom, true, got = load_field_layout(nominal), load_field_layout(built_), load_field_layout(rep["layout"])
    moved_ok = []
    for i in MOVED:
        d0, d1 = K.tag_distance(nom[i], true[i]), K.tag_distance(got[i], true[i])
        c0, c1 = _corner_distance(nom[i], true[i]), _corner_distance(got[i], true[i])
        print("tag", i, "sightings", rep["tags"][i]["sightings"], "nominal to rendered (m, rad)", d0, "corners", c0, "calibrated", d1, "corners", c1,
              "moved", rep["tags"][i]["moved"], "spread", rep["tags"][i].get("std"))
        moved_ok.append(d1[0] < d0[0] and c1 < c0)
    print("rms", rep["rms"], "iters", rep["iters"], "worst tag rms", max(t["rms"] for t in rep["tags"].values()))
    # scipy on the same observations from the same kind of start (the host rig solver's poses with the nominal layout)
    where = {i: k for k, i in enumerate(fc.ids)}
    steps = [[([where[i] for i in ids], b) for ids, b in cams] for cams in obs]
    mounts = [(Am, -Am.T @ b) for Am, b in (rigcal.iso_matrix(m) for m in fc.mounts)]
    solver = RigSolver()
    solver.params.sign_change_error = 0.0
    rr = solver.solve_host([[([fc.layout0[k] for k in ids], b, m) for (ids, b), m in zip(cams, fc.mounts)] for cams in steps], [p[2] for p in poses[:12]])
    ok = [s for s in range(12) if rr[s]["valid"]]
    prob = N.Problem([steps[s] for s in ok], mounts, len(fc.ids))
    sp = rigcal.start_poses(rr)
    p0 = [(sp[ok[u], :9].reshape(3, 3), sp[ok[u], 9:]) for u in prob.used]
    lay0 = [(N.quat_to_mat(list(t.q)), np.array(list(t.t))) for t in fc.layout0]
    free = [[bool(prob.sightings[k] > 0 and fc.ids[k] not in frozen)] * 6 for k in range(len(fc.ids))]
    trf, lm = N.solve(prob, lay0, p0, free)[0], N.solve(prob, lay0, p0, free, method="lm")[0]
    seen = [k for k in range(len(fc.ids)) if prob.sightings[k] > 0]
    mine = [(N.quat_to_mat(list(got[i].q)), np.array(list(got[i].t))) for i in fc.ids]
    d, ref = N.layout_distance(mine, trf, seen), N.layout_distance(trf, lm, seen)
    print("frozen", frozen, "to scipy trf", d, "trf to lm", ref, "bound", 100 * ref)
    # the held-out instants
    held = [f[12:] for f in frames]
    before = _fused_error(tasks, held, poses[12:])
    after = _fused_error(_e2e_tasks(rep["layout"], 16), held, poses[12:])
    print("held-out fused pose error (m, rad): nominal layout", before, "calibrated", after)
    assert all(moved_ok) and len(prob.used) == rep["n_steps_used"] and d <= 100 * ref and after[0] < before[0]
