"""The rig pose refinement on the device (k_rig_refine, chalkydri_amd/csrc/k_rig_refine.hip): ck_rig_refine_batch against
its host twin byte for byte at the shapes where the lanes' loop and the butterfly can go wrong, determinism, ck_rig_process_last_refined
end to end on the two rendered cameras of tests/test_gpu_rig.py, and misuse on the device path."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_rig as N  # noqa: E402
import np_rig_refine as F  # noqa: E402
import scenes  # noqa: E402
from test_gpu_rig import CAMS, rig_scene  # noqa: E402,F401
from test_gpu_rig_robust import SWAP, _swapped  # noqa: E402
from test_rig_refine_host import misuse, to_step  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd.rig import REFINED_DTYPE, RESULT_DTYPE, ROBUST_RESULT_DTYPE, AprilTagsRig, RefineParams, RigSolver, RobustParams, pack_steps  # noqa: E402
from chalkydri_amd.rigcal import last_pose_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
GYRO_SIGMA = 0.01
HEADING_TOL = 1e-9   # the device's cosine and sine of the heading against the host's: see test_process_last_refined


@pytest.fixture(scope="module")
def det(built):
    from chalkydri_amd.detector import AprilTagDetector
    d = AprilTagDetector(64, 64)
    yield d
    d.close()


# 0 tags (no start), 1 tag (4 points), 4 (16), 16 and 17 (exactly one round of the lanes, one round plus four lanes), 8 cameras of one
# tag, one camera of 64 tags, a camera without tags between two that have some
SHAPES = [[0], [1], [4], [16], [17], [1] * 8, [64], [2, 0, 3]]


@pytest.fixture(scope="module")
def shapes(built):
    """per shape: the steps of a batch of one, the heading, the fused start of the twin, masks that delete the last tag of every
    camera with more than one"""
    rng = np.random.default_rng(21)
    s, out = RigSolver(), []
    for counts in SHAPES:
        cams = F.instant(counts, rng)
        gyro = F.TRUTH[2] + rng.normal(0, GYRO_SIGMA)
        start = s.solve_host([to_step(cams)], [gyro])
        assert bool(start["valid"][0]) == (sum(counts) > 0)
        rej = np.zeros((1, A.CK_RIG_MAX_CAMS), np.uint64)
        for c, k in enumerate(counts):
            if k > 1:
                rej[0, c] = 1 << (k - 1)
        out.append((counts, cams, gyro, start, rej))
    return out


def call(L, h, prm, steps, gyro, start, rej):
    """ck_rig_refine_host (h None) or ck_rig_refine_batch with explicit masks"""
    n = len(steps)
    n_cams, probs, tarr, nt, barr = pack_steps(steps)
    g = np.ascontiguousarray(gyro, np.float64)
    st = np.ascontiguousarray(start)
    out = np.zeros(n, REFINED_DTYPE)
    args = [C.byref(prm), n_cams, probs, n, tarr, nt, barr.ctypes.data, len(barr), g.ctypes.data, st.ctypes.data,
            None if rej is None else np.ascontiguousarray(rej).ctypes.data, out.ctypes.data_as(C.POINTER(A.RigRefined))]
    rc = L.ck_rig_refine_host(*args) if h is None else L.ck_rig_refine_batch(h, *args)
    assert rc == A.CK_OK
    return out


CONFIGS = [(planar, gs, masked) for planar in (False, True) for gs in (0.0, GYRO_SIGMA) for masked in (False, True)]


@pytest.mark.parametrize("planar,gs,masked", CONFIGS)
def test_device_matches_twin(det, shapes, planar, gs, masked):
    """Fails without the feature (the symbols are missing).  Every shape as a batch of one, then all of them in one batch of eight
    cameras: the device's records are the twin's bytes."""
    L = det._L
    prm = RefineParams(planar=planar, sigma=F.NOISE, gyro_sigma=gs, max_iters=30)._c(L)
    posed = 0
    for counts, cams, gyro, start, rej in shapes:
        step = [to_step(cams)]
        want = call(L, None, prm, step, [gyro], start, rej if masked else None)
        got = call(L, det._h, prm, step, [gyro], start, rej if masked else None)
        assert got.tobytes() == want.tobytes(), (counts, got, want)
        used = sum(k - (masked and k > 1) for k in counts)
        assert want["n_points"][0] == 4 * used and want["status"][0] == (A.CK_RIG_REFINE_NO_START if not sum(counts) else want["status"][0])
        posed += want["status"][0] <= A.CK_RIG_REFINE_MAXITERS
    assert posed >= len(SHAPES) - 2
    # one batch mixing all of them, every instant padded to eight cameras; the starts are the padded instants' own
    rng = np.random.default_rng(22)
    s = RigSolver()
    steps = [to_step(F.instant(counts, rng, 8)) for counts in SHAPES]
    gyro = [sh[2] for sh in shapes]
    start = s.solve_host(steps, gyro)
    rej = np.concatenate([sh[4] for sh in shapes]) if masked else None
    want = call(L, None, prm, steps, gyro, start, rej)
    got = call(L, det._h, prm, steps, gyro, start, rej)
    assert got.tobytes() == want.tobytes()
    assert want["status"][0] == A.CK_RIG_REFINE_NO_START and (want["status"][1:] != A.CK_RIG_REFINE_NO_START).all()


def test_determinism_and_workspace_reuse(det, shapes):
    """the same call twice gives the same bytes; a small call after a larger one (the workspace stays) and the larger one again too"""
    L = det._L
    prm = RefineParams(planar=True, sigma=F.NOISE, gyro_sigma=GYRO_SIGMA)._c(L)
    big, small = shapes[6], shapes[1]
    a = call(L, det._h, prm, [to_step(big[1])], [big[2]], big[3], None)
    b = call(L, det._h, prm, [to_step(small[1])], [small[2]], small[3], None)
    assert call(L, det._h, prm, [to_step(big[1])], [big[2]], big[3], None).tobytes() == a.tobytes()
    assert call(L, det._h, prm, [to_step(small[1])], [small[2]], small[3], None).tobytes() == b.tobytes()
    assert b.tobytes() == call(L, None, prm, [to_step(small[1])], [small[2]], small[3], None).tobytes()
    # the Python layer: solve_batch(refine=) is solve_batch, then refine_batch
    s = RigSolver(det)
    res, ref = s.solve_batch([to_step(small[1])], [small[2]], refine=RefineParams(planar=True, sigma=F.NOISE, gyro_sigma=GYRO_SIGMA))
    assert ref.tobytes() == s.refine_host([to_step(small[1])], [small[2]], res, RefineParams(planar=True, sigma=F.NOISE, gyro_sigma=GYRO_SIGMA)).tobytes()


def test_misuse_on_the_device_path(det, shapes):
    L = det._L

    def run(p, n_cams, probs, n, tarr, nt, barr, nb, g, st, out, h=det._h):
        return L.ck_rig_refine_batch(h, None if p is None else C.byref(p), n_cams, probs, n, tarr, nt, None if barr is None else barr.ctypes.data, nb,
                                     None if g is None else g.ctypes.data, None if st is None else st.ctypes.data, None,
                                     None if out is None else out.ctypes.data_as(C.POINTER(A.RigRefined)))
    misuse(run, RigSolver())
    counts, cams, gyro, start, rej = shapes[2]
    n_cams, probs, tarr, nt, barr = pack_steps([to_step(cams)])
    p = RefineParams()._c(L)
    out = np.zeros(1, REFINED_DTYPE)
    assert run(p, n_cams, probs, 1, tarr, nt, barr, len(barr), None, start, out, h=None) == A.CK_EINVAL
    with pytest.raises(RuntimeError):
        RigSolver().refine_batch([to_step(cams)], [gyro], start)


def _process_last_refined(tasks, n, gyro, robust, fprm, has=None):
    L = tasks[0].detector._L
    rprm = (robust or RobustParams())._c(L, RigSolver(rig_id=42).params)
    g = np.array(gyro, float)
    has = np.ones(n, np.uint8) if has is None else np.array(has, np.uint8)
    start = np.zeros(n, ROBUST_RESULT_DTYPE if robust else RESULT_DTYPE)
    out = np.zeros(n, REFINED_DTYPE)
    meas, valid = (A.VisionMeasurement * n)(), (C.c_int32 * n)()
    hs = (C.c_void_p * len(tasks))(*[t.detector._h.value for t in tasks])
    rc = L.ck_rig_process_last_refined(hs, len(tasks), n, C.byref(rprm), int(robust is not None), None if fprm is None else C.byref(fprm),
                                       g.ctypes.data, has.ctypes.data, start.ctypes.data, out.ctypes.data_as(C.POINTER(A.RigRefined)), meas, valid)
    return rc, start, out, meas, valid


def _unrefined(tasks, n, gyro, robust, has):
    L = tasks[0].detector._L
    g, has = np.array(gyro, float), np.array(has, np.uint8)
    meas, valid = (A.VisionMeasurement * n)(), (C.c_int32 * n)()
    hs = (C.c_void_p * len(tasks))(*[t.detector._h.value for t in tasks])
    if robust:
        prm = robust._c(L, RigSolver(rig_id=42).params)
        res = np.zeros(n, ROBUST_RESULT_DTYPE)
        rc = L.ck_rig_process_last_robust(hs, len(tasks), n, C.byref(prm), g.ctypes.data, has.ctypes.data, res.ctypes.data_as(C.POINTER(A.RigRobustResult)), meas, valid)
    else:
        prm = RigSolver(rig_id=42).params
        res = np.zeros(n, RESULT_DTYPE)
        rc = L.ck_rig_process_last(hs, len(tasks), n, C.byref(prm), g.ctypes.data, has.ctypes.data, res.ctypes.data_as(C.POINTER(A.RigResult)), meas, valid)
    assert rc == A.CK_OK
    return res, meas, valid


def _close(got, want, tol):
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["n_points"], want["n_points"]) and np.array_equal(got["dof"], want["dof"])
    d = max(np.abs(got["rot"] - want["rot"]).max(), np.abs(got["pos"] - want["pos"]).max())
    ds = np.abs(got["std_devs"] / np.where(want["std_devs"] > 0, want["std_devs"], 1) - (want["std_devs"] > 0)).max()
    print("device heading path against the stand-alone call: pose %.2e, std_devs relative %.2e" % (d, ds))
    assert d < tol and ds < 1e-6


def test_process_last_refined(rig_scene):  # noqa: F811
    """The scene of tests/test_gpu_rig.py through ck_rig_process_last_refined, plain and robust (camera 0's task is then handed the
    layout of tests/test_gpu_rig_robust.py, in which the tag it always sees has changed places with a distant one): start_out is the
    unrefined call's record byte for byte; out is ck_rig_refine_batch on ck_last_pose_inputs' arrays from those records, within
    HEADING_TOL (the device takes the heading's cosine and sine itself; without the prior the bytes are the same); meas carries the
    refined numbers; a step without a heading publishes the fused (blank) measurement; the wrong tag is not in the refined cost."""
    from chalkydri_amd.apriltags import AprilTags
    good, steps = rig_scene
    n = len(steps)
    layout = scenes.wall_layout(12)
    gyro = [s["gyro"] for s in steps]
    has = [1, 1, 1, 0]
    frames = [np.stack([s["views"][c]["frame"] for s in steps]) for c in range(2)]
    for robust in (None, RobustParams()):
        tasks = [AprilTags(w, h, _swapped(layout, *SWAP) if (c == 0 and robust) else layout, scenes.pinhole_calib(f, w / 2.0, h / 2.0), r2c, cam_id=c,
                           max_batch=4) for c, (w, h, f, r2c) in enumerate(CAMS)]
        for t, f in zip(tasks, frames):
            t.process_batch(f, gyro)
        L = tasks[0].detector._L
        res, meas0, valid0 = _unrefined(tasks, n, gyro, robust, has)
        inputs = [last_pose_inputs(t.detector, n)[0] for t in tasks]
        stand = [[(inputs[c][i][0], inputs[c][i][1], tasks[c].robot_to_cam) for c in range(2)] for i in range(n)]
        solver = RigSolver(tasks[0].detector)
        for planar, gs in ((False, 0.0), (True, GYRO_SIGMA)):
            rp = RefineParams(planar=planar, gyro_sigma=gs, max_iters=30)
            rc, start, out, meas, valid = _process_last_refined(tasks, n, gyro, robust, rp._c(L), has)
            assert rc == A.CK_OK and start.tobytes() == res.tobytes() and list(valid) == list(valid0) == [1, 1, 1, 0]
            want = solver.refine_batch(stand, gyro, res, rp)
            if gs == 0.0:
                assert out.tobytes() == want.tobytes()
            else:
                _close(out, want, HEADING_TOL)
            fused = res["fused"] if robust else res
            for i in range(n):
                m, m0 = meas[i], meas0[i]
                assert (m.camera_id, m.tag_count, m.ts) == (m0.camera_id, m0.tag_count, m0.ts) and m.camera_id == 42
                if not has[i]:
                    assert out[i]["status"] == A.CK_RIG_REFINE_NO_START and bytes(m) == bytes(m0) and not fused[i]["valid"]
                    continue
                assert out[i]["status"] <= A.CK_RIG_REFINE_MAXITERS
                assert (m.pose_x, m.pose_y) == (out[i]["pos"][0], out[i]["pos"][1]) and abs(m.pose_rot - np.arctan2(out[i]["rot"][1, 0], out[i]["rot"][0, 0])) < 1e-12
                assert (m.std_x, m.std_y, m.std_rot) == tuple(out[i]["std_devs"])
                x, y, yaw = steps[i]["pose"]
                assert abs(m.pose_x - x) < 0.03 and abs(m.pose_y - y) < 0.03 and abs(m.pose_rot - yaw) < 0.03
                if robust:                           # the planted tag's four corners are absent from the cost
                    assert res[i]["n_rejected"] == 1 and out[i]["n_points"] == 4 * fused[i]["n_tags"] == 4 * (sum(len(inputs[c][i][0]) for c in range(2)) - 1)
                    assert out[i]["rms"] < 0.01
        # the Python layer publishes the same
        rig = AprilTagsRig(tasks, rig_id=42, robust=robust, refine=RefineParams(planar=True, gyro_sigma=GYRO_SIGMA, max_iters=30))
        recs, valid, _ = rig.process_batch(frames, [g if h else None for g, h in zip(gyro, has)])
        assert rig.last_refined.tobytes() == out.tobytes() and bytes(recs) == bytes(meas) and rig.last_results.tobytes() == res.tobytes()
        # misuse: a wrong call count, a null handle, null parameters, bad refinement parameters
        fp = RefineParams()._c(L)
        assert _process_last_refined(tasks, n - 1, gyro[:-1], robust, fp)[0] == A.CK_EINVAL
        assert _process_last_refined(tasks, n, gyro, robust, None)[0] == A.CK_EINVAL
        fp.max_iters = 0
        assert _process_last_refined(tasks, n, gyro, robust, fp)[0] == A.CK_EINVAL
        hs = (C.c_void_p * 2)(tasks[0].detector._h.value, None)
        rprm = RobustParams()._c(L, RigSolver().params)
        fp.max_iters = 10
        assert L.ck_rig_process_last_refined(hs, 2, n, C.byref(rprm), 0, C.byref(fp), np.zeros(n).ctypes.data, np.ones(n, np.uint8).ctypes.data, None,
                                             np.zeros(n, REFINED_DTYPE).ctypes.data_as(C.POINTER(A.RigRefined)), (A.VisionMeasurement * n)(),
                                             (C.c_int32 * n)()) == A.CK_EINVAL
        for t in tasks:
            t.detector.close()
