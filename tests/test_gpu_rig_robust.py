"""The robust camera rig on the device (k_rig_robust, chalkydri_amd/csrc/k_rigpnp.hip): ck_rig_solve_robust_batch on
scenes with planted outliers against the plain solver (poisoned, clean, and with the planted tags deleted) and against its host
twin, ck_rig_process_last_robust end to end on two rendered cameras of which one was handed a field layout with two tags swapped,
misuse, determinism.  The cases are tests/np_rig_robust.py's: tests/test_rig_robust_host.py asserts on the CPU that GNC-TLS recovers
exactly the planted tags on every one of them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_rig as N  # noqa: E402
import np_rig_robust as NR  # noqa: E402
import scenes  # noqa: E402
from test_gpu_rig import CAMS, rig_scene  # noqa: E402,F401  (the rendered two-camera scene, a module-scoped fixture)
from test_rig_robust_host import masks, misuse, to_step  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd.rig import ROBUST_RESULT_DTYPE, AprilTagsRig, RigSolver, RobustParams  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9                     # tests/test_gpu_rig.py's TOL and its bound on the energy (relative)


@pytest.fixture(scope="module")
def det(built):
    from chalkydri_amd.detector import AprilTagDetector
    d = AprilTagDetector(64, 64)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cases():
    return NR.suite()


def _steps(v, key="cams"):
    return [to_step(c[key]) for c in v], [c["gyro"] for c in v]


@pytest.fixture(scope="module")
def robust(det, cases):
    """ck_rig_solve_robust_batch on every group of cases (a call has one number of cameras), once"""
    s = RigSolver(det)
    return {k: s.solve_batch(*_steps(v), robust=True) for k, v in cases.items()}


def test_wrong_tags_are_dropped(det, cases, robust):
    """Fails without the feature: a planted wrong id throws the plain pose by more than gate_rad x (the distance to the nearest tag)
    on every instant that has one (or leaves it without a pose), and the robust pose is the plain solver's on the input with the
    planted tags deleted; the rejected masks are the planted ones exactly, whatever the kind."""
    s = RigSolver(det)
    n = n_id = 0
    for k, v in cases.items():
        poisoned, clean, deleted = s.solve_batch(*_steps(v)), s.solve_batch(*_steps(v, "clean")), None
        deleted = s.solve_batch([to_step(NR.delete_planted(c)) for c in v], [c["gyro"] for c in v])
        for c, p, q, d, got in zip(v, poisoned, clean, deleted, robust[k]):
            if not any(c["planted"]):
                continue
            n += 1
            assert q["valid"] and d["valid"]
            if "id" in c["kinds"] or "behind" in c["kinds"]:
                n_id += 1
                near = min(np.linalg.norm(t - q["pos"]) for tags, _, _ in c["clean"] for _, t in tags)
                off = np.linalg.norm(p["pos"] - q["pos"]) if p["valid"] else np.inf
                print(k, c["kinds"], "plain pose off by", off, "m; bound", NR.GATE * near)
                assert off > NR.GATE * near
            f = got["fused"]
            assert masks(got, k) == c["planted"] and got["status"] == A.CK_RIG_ROBUST_REJECTED and got["rounds"] > 0
            assert f["valid"] == 1 and f["n_tags"] == d["n_tags"] and np.array_equal(f["cam_tags"], d["cam_tags"])
            assert np.abs(f["rot"] - d["rot"]).max() < TOL and np.abs(f["pos"] - d["pos"]).max() < TOL and abs(f["yaw"] - d["yaw"]) < TOL
            assert abs(f["energy"] - d["energy"]) <= TOL * abs(d["energy"])
    assert n >= 25 and n_id >= 12


def test_clean_input_is_the_plain_solve(det, cases, robust):
    s, n = RigSolver(det), 0
    for k, v in cases.items():
        plain = s.solve_batch(*_steps(v))
        for c, p, got in zip(v, plain, robust[k]):
            if any(c["planted"]):
                continue
            n += 1
            assert p["valid"] and got["fused"].tobytes() == p.tobytes()
            assert (got["status"], got["rounds"], got["n_rejected"]) == (A.CK_RIG_ROBUST_CLEAN, 0, 0) and masks(got, k) == [0] * k
    assert n >= 10


def _against_twin(got, want):
    worst = 0.0
    for k in ("status", "rounds", "n_rejected", "rejected"):
        assert np.array_equal(got[k], want[k]), k
    g, w = got["fused"], want["fused"]
    for k in ("valid", "n_tags", "cam_tags"):
        assert np.array_equal(g[k], w[k]), k
    for k in ("rot", "pos", "yaw", "std_devs", "cam_rms"):
        worst = max(worst, np.abs(np.where(g[k] == w[k], 0.0, g[k] - w[k])).max())     # (DBL_MAX standard deviations are equal, not close)
    assert np.all(np.abs(g["energy"] - w["energy"]) <= 1e-9 * np.abs(w["energy"]) + 1e-12)
    for k in ("worst_inlier_rad", "best_rejected_rad"):
        worst = max(worst, np.abs(got[k] - want[k]).max())
    return worst


def test_device_matches_twin(det, cases, robust):
    host, worst = RigSolver(), 0.0
    for k, v in cases.items():
        worst = max(worst, _against_twin(robust[k], host.solve_host(*_steps(v), robust=True)))
    print("device vs twin: worst", worst)
    assert worst < TOL


def test_edges_match_twin(det, cases):
    """an empty step between two others; min_inlier_tags above the survivors (NO_CONSENSUS, with and without a round); one round
    fewer than the weights need (MAXROUNDS)"""
    dev, host = RigSolver(det), RigSolver()
    c = cases[3][0]
    step = to_step(c["cams"])
    empty = [([], np.zeros((0, 3)), m) for _, _, m in step]
    steps, gyro = [step, empty, to_step(cases[3][3]["cams"])], [c["gyro"], 0.0, cases[3][3]["gyro"]]
    full = dev.solve_batch(steps, gyro, robust=True)
    assert full[1].tobytes() == bytes(full[1].nbytes) and full[0]["status"] == A.CK_RIG_ROBUST_REJECTED
    assert full[2]["status"] == A.CK_RIG_ROBUST_CLEAN and full[2]["fused"]["valid"]
    n_in = int(full[0]["fused"]["n_tags"])
    for prm in (RobustParams(), RobustParams(min_inlier_tags=n_in + 1), RobustParams(min_inlier_tags=100),
                RobustParams(max_rounds=int(full[0]["rounds"]) - 1), RobustParams(max_rounds=1), RobustParams(gate_rad=0.02, mu_factor=2.0)):
        got, want = dev.solve_batch(steps, gyro, robust=prm), host.solve_host(steps, gyro, robust=prm)
        assert _against_twin(got, want) < TOL
    got = dev.solve_batch(steps, gyro, robust=RobustParams(min_inlier_tags=n_in + 1))
    assert got[0]["status"] == A.CK_RIG_ROBUST_NO_CONSENSUS and got[0]["fused"].tobytes() == bytes(got[0]["fused"].nbytes)
    assert masks(got[0], 3) == c["planted"] and got[1].tobytes() == bytes(got[1].nbytes)
    got = dev.solve_batch(steps, gyro, robust=RobustParams(min_inlier_tags=100))
    assert got[2]["status"] == A.CK_RIG_ROBUST_NO_CONSENSUS and got[2]["rounds"] == 0 and not got[2]["fused"]["valid"]
    got = dev.solve_batch(steps, gyro, robust=RobustParams(max_rounds=int(full[0]["rounds"]) - 1))
    assert got[0]["status"] == A.CK_RIG_ROBUST_MAXROUNDS and got[0]["fused"]["valid"]
    assert dev.solve_batch([], [], robust=True).shape == (0,)


def test_misuse(det):
    L = det._L

    def call(p, n_cams, probs, n, tarr, nt, barr, g):
        res = np.zeros(max(n, 1), ROBUST_RESULT_DTYPE)
        return L.ck_rig_solve_robust_batch(det._h, None if p is None else C.byref(p), n_cams, probs, n, tarr, nt, barr.ctypes.data,
                                           len(barr), g.ctypes.data, res.ctypes.data_as(C.POINTER(A.RigRobustResult)))
    misuse(call)
    p = A.RigRobustParams()
    L.ck_rig_robust_params_default(C.byref(p))
    res = np.zeros(1, ROBUST_RESULT_DTYPE)
    assert L.ck_rig_solve_robust_batch(None, C.byref(p), 1, (A.SqpnpProblem * 1)(), 0, None, 0, None, 0, np.zeros(1).ctypes.data,
                                       res.ctypes.data_as(C.POINTER(A.RigRobustResult))) == A.CK_EINVAL


def test_determinism(det, cases, robust):
    again = RigSolver(det).solve_batch(*_steps(cases[8]), robust=True)
    assert again.tobytes() == robust[8].tobytes() and again["n_rejected"].any()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
SWAP = (12, 2)       # camera 0 sees tag 12 at every step of the scene and never tag 2; the two are 1.86 m apart on the wall


def _swapped(layout, a, b):
    out = {"tags": [dict(t) for t in layout["tags"]], "field": layout["field"]}
    by_id = {t["ID"]: t for t in out["tags"]}
    by_id[a]["pose"], by_id[b]["pose"] = by_id[b]["pose"], by_id[a]["pose"]
    return out


def _process_last(tasks, n, prm, gyro=None):
    L = tasks[0].detector._L
    g, has = np.zeros(max(n, 1)) if gyro is None else np.array(gyro, float), np.ones(max(n, 1), np.uint8)
    res = np.zeros(max(n, 1), ROBUST_RESULT_DTYPE)
    meas, valid = (A.VisionMeasurement * max(n, 1))(), (C.c_int32 * max(n, 1))()
    hs = (C.c_void_p * len(tasks))(*[t.detector._h.value for t in tasks])
    rc = L.ck_rig_process_last_robust(hs, len(tasks), n, None if prm is None else C.byref(prm), g.ctypes.data, has.ctypes.data,
                                      res.ctypes.data_as(C.POINTER(A.RigRobustResult)), meas, valid)
    return rc, res.tobytes() + bytes(meas) + bytes(valid)


def test_end_to_end(rig_scene):  # noqa: F811
    """The scene of tests/test_gpu_rig.py; camera 0's task is handed a field layout in which tag 12, which it sees at every step,
    and the distant tag 2 have changed places.  The fused measurement is the robust stand-alone solve's on the same inputs, tag 12's
    bit is set in camera 0's mask, and a step without a gyro heading has no pose."""
    from chalkydri_amd.apriltags import AprilTags
    good, steps = rig_scene
    layout = scenes.wall_layout(12)
    tasks = [AprilTags(w, h, _swapped(layout, *SWAP) if c == 0 else layout, scenes.pinhole_calib(f, w / 2.0, h / 2.0), r2c, cam_id=c, max_batch=4)
             for c, (w, h, f, r2c) in enumerate(CAMS)]
    rig = AprilTagsRig(tasks, rig_id=42, robust=True)
    gyro = [s["gyro"] for s in steps]
    gyro[3] = None
    frames = [np.stack([s["views"][c]["frame"] for s in steps]) for c in range(2)]
    recs, valid, _ = rig.process_batch(frames, gyro)
    # the inputs of the stand-alone solve: the fixture's, with the poses camera 0's task was given (ids by their pose in the true layout)
    inputs = []
    for s in steps:
        views = []
        for c in range(2):
            tags, b, mount = s["views"][c]["input"]
            ids = [next(i for i, p in good[c].tags.items() if bytes(p) == bytes(t)) for t in tags]
            views.append(([tasks[c].tags[i] for i in ids], b, mount))
            if c == 0:
                assert SWAP[0] in ids and SWAP[1] not in ids
                s["bit"] = 1 << ids.index(SWAP[0])
        inputs.append(views)
    want = RigSolver().solve_host(inputs, [g or 0.0 for g in gyro], robust=True)
    plain = RigSolver().solve_host(inputs, [g or 0.0 for g in gyro])
    assert list(valid) == [True, True, True, False]
    for i, s in enumerate(steps):
        r, full = recs[i], rig.last_results[i]
        assert r.camera_id == 42
        if gyro[i] is None:
            blank = A.VisionMeasurement()
            blank.camera_id = 42
            assert bytes(r) == bytes(blank) and full.tobytes() == bytes(full.nbytes)
            continue
        w = want[i]
        assert w["fused"]["valid"] and full["fused"]["valid"]
        assert int(full["rejected"][0]) == s["bit"] == int(w["rejected"][0]) and not full["rejected"][1:].any() and full["n_rejected"] == 1
        assert (full["status"], full["rounds"]) == (A.CK_RIG_ROBUST_REJECTED, w["rounds"])
        assert abs(r.pose_x - w["fused"]["pos"][0]) < 1e-6 and abs(r.pose_y - w["fused"]["pos"][1]) < 1e-6
        assert abs(r.pose_rot - w["fused"]["yaw"]) < 1e-7
        assert (r.pose_x, r.pose_y, r.pose_rot) == (full["fused"]["pos"][0], full["fused"]["pos"][1], full["fused"]["yaw"])
        assert np.allclose([r.std_x, r.std_y, r.std_rot], w["fused"]["std_devs"], rtol=1e-6)
        assert r.tag_count == s["views"][0]["n_dets"] + s["views"][1]["n_dets"]          # still all the detections
        x, y, yaw = s["pose"]
        assert abs(r.pose_x - x) < 0.03 and abs(r.pose_y - y) < 0.03 and abs((r.pose_rot - yaw + np.pi) % (2 * np.pi) - np.pi) < 0.03
        assert np.hypot(plain[i]["pos"][0] - x, plain[i]["pos"][1] - y) > 0.03          # ... which the plain fusion of these inputs misses
    # misuse, and the same bytes twice
    p = A.RigRobustParams()
    tasks[0].detector._L.ck_rig_robust_params_default(C.byref(p))
    a, b = _process_last(tasks, 4, p), _process_last(tasks, 4, p)
    assert a[0] == b[0] == A.CK_OK and a[1] == b[1]
    assert _process_last(tasks, 3, p)[0] == A.CK_EINVAL and _process_last(tasks, 4, None)[0] == A.CK_EINVAL
    p.mu_factor = 1.0
    assert _process_last(tasks, 4, p)[0] == A.CK_EINVAL
    for t in tasks:
        t.detector.close()
