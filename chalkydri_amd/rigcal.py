"""Calibration of the camera mounts of a rig: the robot_to_cam of every free camera and one robot pose per step from
a capture of instants in which two or more cameras see field tags, over the C ABI's ck_rigcal_* entry points.

The module functions mirror calibration.py's: `refine_host` (the one-thread twin, the specification), `refine_batch` (all problems
of a call in one launch on a handle's device, the same bytes), `jacobian`, `check`.  MountCalibrator collects steps and solves them
with start poses from the rig solver, the whole capture and, with leave_out = K, K random half-subsets in the same device call.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._lib import check as _check, lib
from .detector import _bind
from .rig import pack_steps

STATUS_NAMES = {A.CK_CALIB_CONVERGED: "converged", A.CK_CALIB_STALLED: "stalled", A.CK_CALIB_MAXIT: "maxit",
                A.CK_CALIB_DEGENERATE: "degenerate"}
ISO_DTYPE = np.dtype([("t", "<f8", (3,)), ("q", "<f8", (4,))])
RESULT_DTYPE = np.dtype([("robot_to_cam", ISO_DTYPE, (A.CK_RIG_MAX_CAMS,)), ("status", "<i4"), ("iters", "<i4"), ("n_steps", "<i4"),
                         ("n_steps_used", "<i4"), ("n_points", "<i4"), ("pad", "<i4"), ("rms", "<f8"), ("cost0", "<f8"), ("cost", "<f8"),
                         ("cam_points", "<i4", (A.CK_RIG_MAX_CAMS,)), ("cam_rms", "<f8", (A.CK_RIG_MAX_CAMS,))])
assert RESULT_DTYPE.itemsize == C.sizeof(A.RigcalResult)


def fix_camera(c):
    """fixed_mask bits of a camera that stays as it is (the gauge needs one such camera)."""
    return 0x3F << (6 * c)


def fix_position(c):
    """fixed_mask bits of a camera whose position in the robot frame was measured: only its angles are solved."""
    return 0x38 << (6 * c)


def params(fixed_mask=fix_camera(0), max_iters=None, min_steps=None, min_cams_per_step=None):
    """ck_rigcal_params_t; None keeps the library's default (100 iterations, 3 steps, 2 cameras per step)."""
    p = A.RigcalParams()
    _bind(lib()).ck_rigcal_params_default(C.byref(p))
    p.fixed_mask = int(fixed_mask)
    for name, v in (("max_iters", max_iters), ("min_steps", min_steps), ("min_cams_per_step", min_cams_per_step)):
        if v is not None:
            setattr(p, name, int(v))
    return p


def _iso(m):
    return m if isinstance(m, A.Iso3) else A.Iso3((C.c_double * 3)(*[float(v) for v in m[0]]), (C.c_double * 4)(*[float(v) for v in m[1]]))


class Capture:
    """The shared arrays of a call.  steps[s][c] = (tags [Iso3], bearings (4 * len(tags), 3)) of camera c at step s (what
    rig.pack_steps takes, without the mount); problems = lists of step numbers, strictly increasing, None = one problem of all steps."""

    def __init__(self, steps, problems=None):
        ident = A.Iso3((C.c_double * 3)(0, 0, 0), (C.c_double * 4)(1, 0, 0, 0))
        self.n_steps = len(steps)
        self.n_cams, self.records, self.tags, self.n_tags, self.bearings = pack_steps([[(v[0], v[1], ident) for v in cams] for cams in steps])
        problems = [list(range(self.n_steps))] if problems is None else [list(q) for q in problems]
        self.n = len(problems)
        self.prob = (A.RigcalProblem * max(self.n, 1))()
        index = []
        for i, q in enumerate(problems):
            self.prob[i].n_steps, self.prob[i].step_offset = len(q), len(index)
            index.extend(q)
        self.step_index = np.array(index + [0], np.int32)
        self.n_index = len(index)

    def capture_args(self):
        return (self.n_cams, self.records, self.n_steps, self.tags, self.n_tags, self.bearings.ctypes.data, len(self.bearings))

    def poses_of(self, poses, i):
        q = self.prob[i]
        return poses[q.step_offset:q.step_offset + q.n_steps]


def _mounts(mounts0):
    return (A.Iso3 * max(len(mounts0), 1))(*[_iso(m) for m in mounts0])


def check(p, cap, mounts0):
    """ck_rigcal_check: the library's return code (0 = the call would be accepted)."""
    return _bind(lib()).ck_rigcal_check(C.byref(p), *cap.capture_args(), cap.prob, cap.n, cap.step_index.ctypes.data, cap.n_index, _mounts(mounts0))


def jacobian(mount, pose, world_xyz, bearings, fixed6=0):
    """ck_rigcal_jacobian: the solver's residuals [n][3] and analytic Jacobian [n][3][12] of one view's points."""
    X, v = np.ascontiguousarray(world_xyz, np.float64).reshape(-1, 3), np.ascontiguousarray(bearings, np.float64).reshape(-1, 3)
    pose = np.ascontiguousarray(pose, np.float64).reshape(12)
    r, J = np.zeros((len(X), 3)), np.zeros((len(X), 3, 12))
    _check(_bind(lib()).ck_rigcal_jacobian(C.byref(_iso(mount)), pose.ctypes.data, X.ctypes.data, v.ctypes.data, len(X), int(fixed6),
                                           r.ctypes.data, J.ctypes.data), "ck_rigcal_jacobian")
    return r, J


def refine_host(p, cap, mounts0, poses0, problem=0):
    """ck_rigcal_refine_host of one problem of the capture, one host thread: (result record, poses [its steps][12])."""
    res, out = np.zeros((), RESULT_DTYPE), np.zeros((max(cap.n_index, 1), 12))
    poses0 = np.ascontiguousarray(poses0, np.float64).reshape(-1, 12)
    if len(poses0) != cap.n_steps:
        raise ValueError("one start pose per step of the capture")
    _check(_bind(lib()).ck_rigcal_refine_host(C.byref(p), *cap.capture_args(), C.byref(cap.prob[problem]), cap.step_index.ctypes.data,
                                              cap.n_index, _mounts(mounts0), poses0.ctypes.data,
                                              C.cast(res.ctypes.data, C.POINTER(A.RigcalResult)), out.ctypes.data), "ck_rigcal_refine_host")
    return res, cap.poses_of(out, problem).copy()


def refine_batch(det, p, cap, mounts0, poses0):
    """ck_rigcal_refine_batch on the detector's handle: (result records [B], list of poses [steps of problem i][12])."""
    res, out = np.zeros(max(cap.n, 1), RESULT_DTYPE), np.zeros((max(cap.n_index, 1), 12))
    poses0 = np.ascontiguousarray(poses0, np.float64).reshape(-1, 12)
    if len(poses0) != cap.n_steps:
        raise ValueError("one start pose per step of the capture")
    _check(_bind(lib()).ck_rigcal_refine_batch(det._h, C.byref(p), *cap.capture_args(), cap.prob, cap.n, cap.step_index.ctypes.data,
                                               cap.n_index, _mounts(mounts0), poses0.ctypes.data,
                                               C.cast(res.ctypes.data, C.POINTER(A.RigcalResult)), out.ctypes.data), "ck_rigcal_refine_batch")
    return res[:cap.n], [cap.poses_of(out, i).copy() for i in range(cap.n)]


def calibrate_batch(det, p, cap, mounts0, gyro):
    """ck_rig_calibrate_batch: the starts from the rig solver on the device (gyro [n_steps], the steps' headings), then the
    refinement of all problems in one launch.  A step the rig solver has no pose for is left out of every problem."""
    res, out = np.zeros(max(cap.n, 1), RESULT_DTYPE), np.zeros((max(cap.n_index, 1), 12))
    g = np.ascontiguousarray(gyro, np.float64).reshape(-1)
    if len(g) != cap.n_steps:
        raise ValueError("one heading per step of the capture")
    g = g if len(g) else np.zeros(1)
    _check(_bind(lib()).ck_rig_calibrate_batch(det._h, C.byref(p), *cap.capture_args(), g.ctypes.data, cap.prob, cap.n,
                                               cap.step_index.ctypes.data, cap.n_index, _mounts(mounts0),
                                               C.cast(res.ctypes.data, C.POINTER(A.RigcalResult)), out.ctypes.data), "ck_rig_calibrate_batch")
    return res[:cap.n], [cap.poses_of(out, i).copy() for i in range(cap.n)]


def last_pose_inputs(det, n):
    """ck_last_pose_inputs: what the detector's last process call of n frames left for the pose solvers, as a list of n
    (tags [Iso3], bearings (4 k, 3)) and the records themselves."""
    L = _bind(lib())
    rec = (A.SqpnpProblem * n)()
    nt, nb = C.c_int32(0), C.c_int32(0)
    one_t, one_b = (A.Iso3 * 1)(), np.zeros((1, 3))
    rc = L.ck_last_pose_inputs(det._h, n, rec, one_t, 0, one_b.ctypes.data, 0, C.byref(nt), C.byref(nb))
    if rc not in (A.CK_OK, A.CK_ECAPACITY):
        _check(rc, "ck_last_pose_inputs")
    tags, bear = (A.Iso3 * max(nt.value, 1))(), np.zeros((max(nb.value, 1), 3))
    _check(L.ck_last_pose_inputs(det._h, n, rec, tags, nt.value, bear.ctypes.data, nb.value, C.byref(nt), C.byref(nb)), "ck_last_pose_inputs")
    steps = []
    for r in rec:
        steps.append(([A.Iso3.from_buffer_copy(tags[r.tag_offset + k]) for k in range(r.n_tags)],
                      bear[r.bearing_offset:r.bearing_offset + r.n_bearings].copy()))
    return steps, rec


def mount_offsets(iso):
    """The reference's RobotToCamOffset {x, y, z, roll, pitch, yaw} (metres, degrees) of a robot_to_cam: the inverse of
    create_solver_camera_transform, on the host.  What AprilTags(..., robot_to_cam=) takes."""
    Am, b = iso_matrix(iso)
    o = -Am.T @ b
    Rn = Am.T @ np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]]).T           # robot <- camera body: Rz(yaw) Ry(pitch) Rx(roll)
    roll, pitch, yaw = np.arctan2(Rn[2, 1], Rn[2, 2]), -np.arcsin(np.clip(Rn[2, 0], -1, 1)), np.arctan2(Rn[1, 0], Rn[0, 0])
    return {"x": float(o[0]), "y": float(o[1]), "z": float(o[2]), "roll": float(np.degrees(roll)), "pitch": float(np.degrees(pitch)),
            "yaw": float(np.degrees(yaw))}


def start_poses(rig_results):
    """World -> robot start poses [n][12] (R row-major, t) from the rig solver's records (rot = world <- robot, pos); a step
    without a pose gets NaN, which leaves a problem that uses it DEGENERATE: drop such steps from the problems."""
    out = np.full((len(rig_results), 12), np.nan)
    for s, r in enumerate(rig_results):
        if r["valid"]:
            R = np.asarray(r["rot"]).T
            out[s, :9], out[s, 9:] = R.reshape(9), -R @ np.asarray(r["pos"])
    return out


def iso_matrix(iso):
    """(A [3][3], b [3]) of a robot_to_cam record (numpy ISO_DTYPE scalar, Iso3 or (t, q))."""
    t, q = (iso["t"], iso["q"]) if isinstance(iso, (np.void, np.ndarray)) else ((iso.t, iso.q) if isinstance(iso, A.Iso3) else iso)
    w, x, y, z = np.asarray(list(q), float) / np.linalg.norm(list(q))
    Am = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return Am, np.asarray(list(t), float)


class MountCalibrator:
    """Collects steps of a rig and solves for the mounts.  rig: an AprilTagsRig, whose tasks give the start mounts and whose first
    detector gives the device and stream; or, without cameras, det = an AprilTagDetector and mounts0 = the start robot_to_cam of every
    camera (Iso3 or (t, q)), the steps then come through add_steps.  fixed: the fixed_mask, by default camera 0 wholly (the gauge)."""

    def __init__(self, rig=None, fixed=None, det=None, mounts0=None):
        self.rig = rig
        self.det = rig.tasks[0].detector if rig is not None else det
        self.mounts0 = [_iso(m) for m in (mounts0 if mounts0 is not None else [t.robot_to_cam for t in rig.tasks])]
        if not 1 <= len(self.mounts0) <= A.CK_RIG_MAX_CAMS:
            raise ValueError(f"a rig has 1..{A.CK_RIG_MAX_CAMS} cameras")
        self.fixed = fix_camera(0) if fixed is None else int(fixed)
        self._steps, self._gyro = [], []

    def process(self, frames_per_camera, gyro):
        """rig.process_batch on frames_per_camera[c] = camera c's frames [n][h][w] with the headings gyro[n], then the steps of the
        call are appended from what it left on the device (ck_last_pose_inputs).  An instant without a heading (None, as
        rig.process_batch takes it: "no gyro, no solve") has no pose inputs and is not kept.  Returns rig.process_batch's result."""
        out = self.rig.process_batch(frames_per_camera, gyro)
        n = len(frames_per_camera[0])
        if n:
            per_cam = [last_pose_inputs(t.detector, n)[0] for t in self.rig.tasks]
            heading = [gyro if (gyro is None or np.isscalar(gyro)) else gyro[s] for s in range(n)]
            keep = [s for s in range(n) if heading[s] is not None]
            self.add_steps([[per_cam[c][s] for c in range(len(per_cam))] for s in keep], [heading[s] for s in keep])
        return out

    def add_steps(self, steps, gyro):
        """steps[s][c] = (tags [Iso3], bearings (4 * len(tags), 3)) of camera c; gyro[s] = the heading of the step (the rig solver's
        start needs it).  Returns the number of steps kept so far."""
        for cams, g in zip(steps, gyro):
            if len(cams) != len(self.mounts0):
                raise ValueError("every step needs one entry per camera")
            self._steps.append([(list(t), np.asarray(b, np.float64).reshape(-1, 3)) for t, b in cams])
            self._gyro.append(float(g))
        return len(self._steps)

    def observations(self):
        return list(self._steps)

    def clear(self):
        self._steps, self._gyro = [], []

    def calibrate(self, fixed_mask=None, leave_out=0, seed=0, max_iters=None):
        """Solves the kept steps (ck_rig_calibrate_batch): a report dict, or None when the solve neither converged nor stalled at a
        finite rms.  Start poses come from the rig solver with the start mounts; steps it cannot solve are left out.  report:
        robot_to_cam (list of (t, q)), offsets (list of {x, y, z, roll, pitch, yaw}: what AprilTags(..., robot_to_cam=) takes), status,
        iters, rms, cam_rms, n_steps_used, poses, and with leave_out = K > 0 `std`, per camera the standard deviation of the six
        offsets over K random half-subsets (those that solved: `n_subsets`), all problems in the same device call."""
        p = params(self.fixed if fixed_mask is None else fixed_mask, max_iters)
        n_steps = len(self._steps)
        if n_steps < p.min_steps:
            return None
        problems, rng = [list(range(n_steps))], np.random.default_rng(seed)
        half = max(p.min_steps, (n_steps + 1) // 2)
        for _ in range(int(leave_out)):
            problems.append(sorted(rng.choice(n_steps, half, replace=False).tolist()))
        cap = Capture(self._steps, problems)
        res, poses = calibrate_batch(self.det, p, cap, self.mounts0, self._gyro)
        ok = lambda r: r["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED) and np.isfinite(r["rms"])
        if not ok(res[0]):
            return None
        n = len(self.mounts0)
        report = {"robot_to_cam": [(res[0]["robot_to_cam"][c]["t"].copy(), res[0]["robot_to_cam"][c]["q"].copy()) for c in range(n)],
                  "offsets": [mount_offsets(res[0]["robot_to_cam"][c]) for c in range(n)],
                  "status": STATUS_NAMES[int(res[0]["status"])], "iters": int(res[0]["iters"]), "rms": float(res[0]["rms"]),
                  "cam_rms": res[0]["cam_rms"][:n].copy(), "n_steps_used": int(res[0]["n_steps_used"]), "poses": poses[0]}
        if leave_out:
            sub = [[mount_offsets(r["robot_to_cam"][c]) for c in range(n)] for r in res[1:] if ok(r)]
            report["n_subsets"] = len(sub)
            report["std"] = [{k: float(np.std([m[c][k] for m in sub])) for k in sub[0][c]} for c in range(n)] if len(sub) > 1 else None
        return report
