"""The camera rig on the device (k_rig, chalkydri_amd/csrc/k_rigpnp.hip): ck_rig_solve_batch against its host twin and
against k_sqpnp for one camera, ck_rig_process_last end to end on two rendered cameras, misuse, determinism.
The kernel's own edges (more than 64 and 128 points, empty cameras in every position, coplanar and singular scenes, candidates behind
a camera, the gyro far off and across +-pi, every branch of std_devs) are pinned by tests/test_gpu_rig_cases.py, against this twin and against tests/np_rig.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_rig as N  # noqa: E402
import scenes  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd import default_config  # noqa: E402
from chalkydri_amd.rig import RESULT_DTYPE, AprilTagsRig, RigSolver  # noqa: E402
from chalkydri_amd.sqpnp import iso3  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9


def to_step(cams):
    return [([iso3(t, N.mat_to_quat(R)) for R, t in tags], b, iso3(bb, N.mat_to_quat(Am))) for tags, b, (Am, bb) in cams]


@pytest.fixture(scope="module")
def det(built):
    from chalkydri_amd.detector import AprilTagDetector
    d = AprilTagDetector(64, 64)
    yield d
    d.close()


def test_device_matches_twin(det):
    """64 problems of test_rig_host's generator, grouped by their number of cameras (1, 2, 3, 4 and 8; a call has one number), with
    a step without any tag and a camera with 3 tags beside one with none among them."""
    rng = np.random.default_rng(20261019)
    groups = {}
    for k in range(64):
        n_cams = (1, 2, 3, 4, 8)[k % 5]
        cams, gyro, _ = N.make_rig(rng, n_cams=n_cams, noise=0.0 if k % 2 == 0 else 1e-3, gyro_noise=0.0 if k % 2 == 0 else 0.02)
        groups.setdefault(n_cams, []).append((to_step(cams), gyro))
    cams, gyro, _ = N.make_rig(rng, n_cams=2, noise=1e-3, tags_per_cam=(3, 3))
    step = to_step(cams)
    groups[2].append(([step[0], ([], np.zeros((0, 3)), step[1][2])], gyro))                 # 3 tags beside none
    groups[2].append(([([], np.zeros((0, 3)), m) for _, _, m in step], gyro))               # no tag at all
    dev, host = RigSolver(det), RigSolver()
    worst = dict.fromkeys(("rot", "pos", "yaw", "std_devs", "cam_rms"), 0.0)
    total = 0
    for n_cams, items in sorted(groups.items()):
        steps, gyros = [s for s, _ in items], [g for _, g in items]
        got, want = dev.solve_batch(steps, gyros), host.solve_host(steps, gyros)
        if n_cams == 2:                                                                     # the two special steps are what they were built as
            assert want[-1]["valid"] == 0 and want[-2]["valid"] == 1 and list(want[-2]["cam_tags"][:2]) == [3, 0]
        assert np.array_equal(got["valid"], want["valid"]) and np.array_equal(got["cam_tags"], want["cam_tags"])
        assert np.array_equal(got["n_tags"], want["n_tags"])
        for g, w in zip(got, want):
            total += 1
            if not w["valid"]:
                assert g.tobytes() == bytes(g.nbytes)
                continue
            for k in worst:
                same = (g[k] == w[k])                                                       # (DBL_MAX standard deviations are equal, not close)
                worst[k] = max(worst[k], np.abs(np.where(same, 0.0, g[k] - w[k])).max())
            assert abs(g["energy"] - w["energy"]) <= 1e-9 * abs(w["energy"]) + 1e-12
    print("device vs twin:", total, "problems,", worst)
    assert total == 66
    assert all(v < TOL for v in worst.values()), worst


def test_one_camera_rig_matches_k_sqpnp(det):
    """16 one-camera problems of 2 or 3 tags: the rig kernel against ck_sqpnp_solve_batch.  (One tag alone: see
    test_rig_host.test_one_camera_rig_is_sqpnp.)  The standard deviations take |t| of the robot where k_sqpnp takes the camera's:
    compared where the mount has no translation (the even problems)."""
    from chalkydri_amd.sqpnp import SqPnP
    rng = np.random.default_rng(11)
    steps, gyros, single = [], [], []
    for i in range(16):
        cams, gyro, _ = N.make_rig(rng, n_cams=1, noise=1e-3, tags_per_cam=(2, 3), gyro_noise=0.02, mount_translation=0.0 if i % 2 == 0 else 0.4)
        step = to_step(cams)
        steps.append(step); gyros.append(gyro)
        single.append((step[0][0], step[0][1], step[0][2], gyro, 600.0))
    got = RigSolver(det).solve_batch(steps, gyros)
    want = SqPnP(det).solve_batch(single)
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["valid"] and w is not None
        worst = max(worst, np.abs(g["rot"] - w["rot"]).max(), np.abs(g["pos"] - w["pos"]).max(), abs(g["yaw"] - w["yaw"]))
        if i % 2 == 0:
            worst = max(worst, np.abs(g["std_devs"] - w["std_devs"]).max())
    print("one-camera rig vs k_sqpnp: worst", worst)
    assert worst < TOL


# ---- end to end -------------------------------------------------------------------------------------------------------------------
CAMS = ((640, 400, 550.0, {"roll": 0.0, "pitch": 0.0, "yaw": 25.0, "x": 0.2, "y": 0.15, "z": 0.6}),
        (800, 600, 700.0, {"roll": 0.0, "pitch": 0.0, "yaw": -25.0, "x": 0.2, "y": -0.15, "z": 0.6}))


@pytest.fixture(scope="module")
def rig_scene(oracle):
    """Two AprilTags tasks of different size looking at a wall of 12 tags from 4 robot poses, chosen on the CPU with the oracle: every
    frame gives a pose of its own (so it holds a known tag) and the two cameras do not see the same set of tags.  Per step and
    camera: the frame, the oracle's detections, the pose inputs (known tags and the bearings of their corners)."""
    from chalkydri_amd.apriltags import AprilTags
    layout = scenes.wall_layout(12)
    tasks = [AprilTags(w, h, layout, scenes.pinhole_calib(f, w / 2.0, h / 2.0), r2c, cam_id=c, max_batch=4)
             for c, (w, h, f, r2c) in enumerate(CAMS)]
    rng = np.random.default_rng(3)
    steps = []
    for attempt in range(40):
        if len(steps) == 4:
            break
        pose = (rng.uniform(1.5, 2.5), rng.uniform(-0.6, 0.6), rng.uniform(-0.25, 0.25))
        gyro = pose[2] + rng.uniform(-0.02, 0.02)
        views, ok = [], True
        for c, (w, h, f, r2c) in enumerate(CAMS):
            frame, truth = scenes.render_view(2000 + 10 * attempt + c, w, h, f, layout, pose, r2c, noise_amp=1)
            out, v = A.VisionMeasurement(), C.c_int(0)
            cfg = default_config(w, h)
            oracle.lib().ora_process_frame(C.c_void_p(frame.ctypes.data), w, h, w, C.byref(cfg), C.byref(tasks[c]._pp), C.c_double(gyro), 1,
                                           C.byref(out), C.byref(v))
            dets, _ = oracle.detect(frame, cfg)
            known = [d for d in dets if d["id"] in tasks[c].tags]
            ok = ok and bool(v.value) and len(known) >= 1
            cam = [getattr(tasks[c].cam, k) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]
            tags, bearings = [], []
            for d in known:
                b, good = oracle.unproject_opencv5(cam, d["p"])
                if good.all():
                    tags.append(tasks[c].tags[d["id"]]); bearings.append(b)
            views.append({"frame": frame, "n_dets": len(dets), "ids": sorted(d["id"] for d in known), "truth": truth,
                          "input": (tags, np.concatenate(bearings) if bearings else np.zeros((0, 3)), tasks[c].robot_to_cam)})
        if ok and views[0]["ids"] != views[1]["ids"]:
            steps.append({"pose": pose, "gyro": gyro, "views": views})
    assert len(steps) == 4
    yield tasks, steps
    for t in tasks:
        t.detector.close()


def test_end_to_end(rig_scene):
    tasks, steps = rig_scene
    rig = AprilTagsRig(tasks, rig_id=42)
    gyro = [s["gyro"] for s in steps]
    gyro[2] = None                                              # "no gyro, no solve"
    frames = [np.stack([s["views"][c]["frame"] for s in steps]) for c in range(2)]
    recs, valid, per_cam = rig.process_batch(frames, gyro)
    want = RigSolver().solve_host([[s["views"][c]["input"] for c in range(2)] for s in steps], [g or 0.0 for g in gyro])
    assert list(valid) == [True, True, False, True]
    for i, s in enumerate(steps):
        r, full = recs[i], rig.last_results[i]
        assert r.camera_id == 42
        if gyro[i] is None:
            blank = A.VisionMeasurement()
            blank.camera_id = 42
            assert bytes(r) == bytes(blank) and full.tobytes() == bytes(full.nbytes)
            continue
        w = want[i]
        assert w["valid"] and full["valid"]
        assert list(full["cam_tags"][:2]) == [len(s["views"][c]["ids"]) for c in range(2)] == list(w["cam_tags"][:2])
        assert abs(r.pose_x - w["pos"][0]) < 1e-6 and abs(r.pose_y - w["pos"][1]) < 1e-6 and abs(r.pose_rot - w["yaw"]) < 1e-7
        assert (r.pose_x, r.pose_y, r.pose_rot) == (full["pos"][0], full["pos"][1], full["yaw"])
        assert np.allclose([r.std_x, r.std_y, r.std_rot], w["std_devs"], rtol=1e-6)
        assert r.tag_count == s["views"][0]["n_dets"] + s["views"][1]["n_dets"]
        x, y, yaw = s["pose"]
        assert abs(r.pose_x - x) < 0.03 and abs(r.pose_y - y) < 0.03 and abs((r.pose_rot - yaw + np.pi) % (2 * np.pi) - np.pi) < 0.03
        for c in range(2):                                     # the per-camera records are what the tasks return on their own
            assert per_cam[c][1][i] and per_cam[c][0][i].camera_id == c


def _process_last(tasks, n, rig_id=42):
    L = tasks[0].detector._L
    prm = RigSolver(rig_id=rig_id).params
    g, has = np.zeros(max(n, 1)), np.ones(max(n, 1), np.uint8)
    res = np.zeros(max(n, 1), RESULT_DTYPE)
    meas, valid = (A.VisionMeasurement * max(n, 1))(), (C.c_int32 * max(n, 1))()
    hs = (C.c_void_p * len(tasks))(*[t.detector._h.value for t in tasks])
    rc = L.ck_rig_process_last(hs, len(tasks), n, C.byref(prm), g.ctypes.data, has.ctypes.data, res.ctypes.data_as(C.POINTER(A.RigResult)), meas, valid)
    return rc, res.tobytes() + bytes(meas) + bytes(valid)


def test_misuse(rig_scene):
    from chalkydri_amd.apriltags import AprilTags
    _, steps = rig_scene
    layout = scenes.wall_layout(12)
    tasks = [AprilTags(w, h, layout, scenes.pinhole_calib(f, w / 2.0, h / 2.0), r2c, cam_id=c, max_batch=4) for c, (w, h, f, r2c) in enumerate(CAMS)]
    frames = [np.stack([s["views"][c]["frame"] for s in steps[:2]]) for c in range(2)]
    assert _process_last(tasks, 2)[0] == A.CK_EINVAL                       # before any process call
    for t, f in zip(tasks, frames):
        t.process_batch(f, [0.0, 0.0])
    assert _process_last(tasks, 3)[0] == A.CK_EINVAL                       # n is not the handles' last call
    assert _process_last(tasks, 2)[0] == A.CK_OK
    tasks[1].detector.detect_batch(frames[1])                              # a plain detect rewrote camera 1's workspace
    assert _process_last(tasks, 2)[0] == A.CK_EINVAL
    tasks[1].process_batch(frames[1], [0.0, 0.0])                          # the handles work afterwards
    rc, _ = _process_last(tasks, 2)
    assert rc == A.CK_OK
    for t in tasks:
        t.detector.close()


def test_determinism(rig_scene, det):
    tasks, steps = rig_scene
    frames = [np.stack([s["views"][c]["frame"] for s in steps]) for c in range(2)]
    for t, f in zip(tasks, frames):
        t.process_batch(f, [s["gyro"] for s in steps])
    a, b = _process_last(tasks, 4), _process_last(tasks, 4)
    assert a[0] == b[0] == A.CK_OK and a[1] == b[1]
    rng = np.random.default_rng(1)
    items = [N.make_rig(rng, n_cams=3, noise=1e-3)[:2] for _ in range(8)]
    s = RigSolver(det)
    r1 = s.solve_batch([to_step(c) for c, _ in items], [g for _, g in items])
    r2 = s.solve_batch([to_step(c) for c, _ in items], [g for _, g in items])
    assert r1.tobytes() == r2.tobytes() and r1["valid"].any()
