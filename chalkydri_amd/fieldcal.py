"""Calibration of the field's tag layout: the world <- tag pose of every tag that is not frozen and one robot pose
per step from a capture of instants in which the cameras see two or more tags, over the C ABI's ck_fieldcal_* entry points.  The
mounts are inputs and stay fixed.

The module functions mirror rigcal.py's: `refine_host` (the one-thread twin, the specification), `refine_batch` (all problems of a
call in one launch on a handle's device, the same bytes), `calibrate_batch` (starts from the rig solver), `jacobian`, `check`.
FieldCalibrator collects steps and solves them, the whole capture and, with leave_out = K, K random half-subsets in the same device
call, and returns the layout in the field.json schema.
"""
import ctypes as C
import json

import numpy as np

from . import _abi as A
from ._lib import check as _check, lib
from .detector import _bind
from .rigcal import ISO_DTYPE, STATUS_NAMES, _iso, _mounts, iso_matrix, last_pose_inputs

RESULT_DTYPE = np.dtype([("status", "<i4"), ("iters", "<i4"), ("n_steps", "<i4"), ("n_steps_used", "<i4"), ("n_points", "<i4"),
                         ("n_tags_solved", "<i4"), ("rms", "<f8"), ("cost0", "<f8"), ("cost", "<f8")])
assert RESULT_DTYPE.itemsize == C.sizeof(A.FieldcalResult)
FIX_ALL, FIX_ROTATION, FIX_POSITION = 0x3F, 0x07, 0x38


def params(max_iters=None, min_steps=None, min_tags_per_step=None):
    """ck_fieldcal_params_t; None keeps the library's default (100 iterations, 3 steps, 2 tags per step)."""
    p = A.FieldcalParams()
    _bind(lib()).ck_fieldcal_params_default(C.byref(p))
    for name, v in (("max_iters", max_iters), ("min_steps", min_steps), ("min_tags_per_step", min_tags_per_step)):
        if v is not None:
            setattr(p, name, int(v))
    return p


class Capture:
    """The shared arrays of a call.  steps[s][c] = (entries of the layout [k], bearings (4 * k, 3)) of camera c at step s;
    problems = lists of step numbers, strictly increasing, None = one problem of all steps."""

    def __init__(self, steps, problems=None):
        self.n_steps = n = len(steps)
        self.n_cams = len(steps[0]) if n else 1
        self.records = (A.SqpnpProblem * max(self.n_cams * n, 1))()
        index, bear, nb = [], [], 0
        for s, cams in enumerate(steps):
            if len(cams) != self.n_cams:
                raise ValueError("every step needs the same number of cameras")
            for c, (ids, b) in enumerate(cams):
                b = np.asarray(b, np.float64).reshape(-1, 3)
                r = self.records[c * n + s]
                r.n_tags, r.n_bearings, r.tag_offset, r.bearing_offset = len(ids), len(b), len(index), nb
                index.extend(int(k) for k in ids)
                bear.append(b)
                nb += len(b)
        self.n_tags = len(index)
        self.tag_index = np.array(index + [0], np.int32)
        self.bearings = np.ascontiguousarray(np.concatenate(bear) if bear else np.zeros((0, 3)), np.float64)
        problems = [list(range(n))] if problems is None else [list(q) for q in problems]
        self.n = len(problems)
        self.prob = (A.RigcalProblem * max(self.n, 1))()
        idx = []
        for i, q in enumerate(problems):
            self.prob[i].n_steps, self.prob[i].step_offset = len(q), len(idx)
            idx.extend(q)
        self.step_index = np.array(idx + [0], np.int32)
        self.n_index = len(idx)

    def capture_args(self):
        return (self.n_cams, self.records, self.n_steps, self.tag_index.ctypes.data, self.n_tags, self.bearings.ctypes.data, len(self.bearings))

    def poses_of(self, poses, i):
        q = self.prob[i]
        return poses[q.step_offset:q.step_offset + q.n_steps]


def _layout(layout0, fixed6):
    arr = (A.Iso3 * max(len(layout0), 1))(*[_iso(t) for t in layout0])
    fx = np.ascontiguousarray(fixed6, np.uint8).reshape(-1)
    if len(fx) != len(layout0):
        raise ValueError("one mask per entry of the layout")
    return arr, len(layout0), (fx if len(fx) else np.zeros(1, np.uint8))


def check(p, cap, mounts, layout0, fixed6):
    """ck_fieldcal_check: the library's return code (0 = the call would be accepted)."""
    lay, n, fx = _layout(layout0, fixed6)
    return _bind(lib()).ck_fieldcal_check(C.byref(p), *cap.capture_args(), cap.prob, cap.n, cap.step_index.ctypes.data, cap.n_index,
                                          _mounts(mounts), lay, n, fx.ctypes.data)


def jacobian(mount, pose, tag, bearings, fixed6=0):
    """ck_fieldcal_jacobian: the solver's residuals [n][3] and analytic Jacobian [n][3][12] of the first n <= 4 corners of one sighting."""
    v = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3)
    pose = np.ascontiguousarray(pose, np.float64).reshape(12)
    r, J = np.zeros((len(v), 3)), np.zeros((len(v), 3, 12))
    _check(_bind(lib()).ck_fieldcal_jacobian(C.byref(_iso(mount)), pose.ctypes.data, C.byref(_iso(tag)), v.ctypes.data, len(v), int(fixed6),
                                             r.ctypes.data, J.ctypes.data), "ck_fieldcal_jacobian")
    return r, J


def _outputs(cap, n_layout, n):
    return (np.zeros(max(n, 1), RESULT_DTYPE), np.zeros((max(n, 1), n_layout), ISO_DTYPE), np.zeros((max(n, 1), n_layout), np.int32),
            np.zeros((max(n, 1), n_layout)), np.zeros((max(cap.n_index, 1), 12)))


def _out_args(res, lay, sight, rms, out):
    return (C.cast(res.ctypes.data, C.POINTER(A.FieldcalResult)), C.cast(lay.ctypes.data, C.POINTER(A.Iso3)), sight.ctypes.data,
            rms.ctypes.data, out.ctypes.data)


def _poses0(cap, poses0):
    poses0 = np.ascontiguousarray(poses0, np.float64).reshape(-1, 12)
    if len(poses0) != cap.n_steps:
        raise ValueError("one start pose per step of the capture")
    return poses0 if len(poses0) else np.zeros((1, 12))


def refine_host(p, cap, mounts, layout0, fixed6, poses0, problem=0):
    """ck_fieldcal_refine_host of one problem of the capture, one host thread: (result record, layout [n_layout] of ISO_DTYPE,
    sightings [n_layout], tag rms [n_layout], poses [its steps][12])."""
    lay0, n, fx = _layout(layout0, fixed6)
    res, lay, sight, rms, out = _outputs(cap, n, 1)
    poses0 = _poses0(cap, poses0)
    _check(_bind(lib()).ck_fieldcal_refine_host(C.byref(p), *cap.capture_args(), C.byref(cap.prob[problem]), cap.step_index.ctypes.data,
                                                cap.n_index, _mounts(mounts), lay0, n, fx.ctypes.data, poses0.ctypes.data,
                                                *_out_args(res, lay, sight, rms, out)), "ck_fieldcal_refine_host")
    return res[0], lay[0], sight[0], rms[0], cap.poses_of(out, problem).copy()


def refine_batch(det, p, cap, mounts, layout0, fixed6, poses0):
    """ck_fieldcal_refine_batch on the detector's handle: (result records [B], layouts [B][n_layout], sightings [B][n_layout], tag rms
    [B][n_layout], list of poses [steps of problem i][12])."""
    lay0, n, fx = _layout(layout0, fixed6)
    res, lay, sight, rms, out = _outputs(cap, n, cap.n)
    poses0 = _poses0(cap, poses0)
    _check(_bind(lib()).ck_fieldcal_refine_batch(det._h, C.byref(p), *cap.capture_args(), cap.prob, cap.n, cap.step_index.ctypes.data,
                                                 cap.n_index, _mounts(mounts), lay0, n, fx.ctypes.data, poses0.ctypes.data,
                                                 *_out_args(res, lay, sight, rms, out)), "ck_fieldcal_refine_batch")
    return res[:cap.n], lay[:cap.n], sight[:cap.n], rms[:cap.n], [cap.poses_of(out, i).copy() for i in range(cap.n)]


def calibrate_batch(det, p, cap, mounts, layout0, fixed6, gyro):
    """ck_field_calibrate_batch: the starts from the rig solver on the device with the tags at layout0 (gyro [n_steps], the steps'
    headings), then the refinement of all problems in one launch.  A step the rig solver has no pose for is left out of every problem."""
    lay0, n, fx = _layout(layout0, fixed6)
    res, lay, sight, rms, out = _outputs(cap, n, cap.n)
    g = np.ascontiguousarray(gyro, np.float64).reshape(-1)
    if len(g) != cap.n_steps:
        raise ValueError("one heading per step of the capture")
    g = g if len(g) else np.zeros(1)
    _check(_bind(lib()).ck_field_calibrate_batch(det._h, C.byref(p), *cap.capture_args(), g.ctypes.data, cap.prob, cap.n,
                                                 cap.step_index.ctypes.data, cap.n_index, _mounts(mounts), lay0, n, fx.ctypes.data,
                                                 *_out_args(res, lay, sight, rms, out)), "ck_field_calibrate_batch")
    return res[:cap.n], lay[:cap.n], sight[:cap.n], rms[:cap.n], [cap.poses_of(out, i).copy() for i in range(cap.n)]


def tag_distance(a, b):
    """(metres, radians) between two tag poses (ISO_DTYPE records, Iso3 or (t, q)); the angle from the skew part of the relative
    rotation, which resolves angles far below the 1e-8 at which arccos of the trace stops."""
    (Ra, ta), (Rb, tb) = iso_matrix(a), iso_matrix(b)
    Rd = Ra.T @ Rb
    w = 0.5 * np.array([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]])
    return float(np.linalg.norm(ta - tb)), float(np.arctan2(np.linalg.norm(w), (np.trace(Rd) - 1) / 2))


def layout_dict(ids, layout, field=None):
    """The reference's field.json schema of a layout: ids [n], layout [n] of ISO_DTYPE records, Iso3 or (t, q); `field` is copied through."""
    tags = []
    for tid, rec in zip(ids, layout):
        t, q = (rec["t"], rec["q"]) if isinstance(rec, (np.void, np.ndarray)) else ((rec.t, rec.q) if isinstance(rec, A.Iso3) else rec)
        tags.append({"ID": int(tid), "pose": {"translation": {"x": float(t[0]), "y": float(t[1]), "z": float(t[2])},
                                              "rotation": {"quaternion": {"W": float(q[0]), "X": float(q[1]), "Y": float(q[2]), "Z": float(q[3])}}}})
    out = {"tags": tags}
    if field is not None:
        out["field"] = field
    return out


class FieldCalibrator:
    """Collects steps of a rig (of one camera or more) and solves for the tag layout.  rig: an AprilTagsRig, whose tasks give the
    mounts, whose first task gives the nominal layout and whose first detector gives the device and stream; or, without cameras,
    det = an AprilTagDetector and mounts = the robot_to_cam of every camera (Iso3 or (t, q)), the steps then come through add_steps.
    layout: the nominal layout, a field.json dict or path or {id: Iso3}; by default the first task's.  fixed: {tag id: mask}
    (FIX_ALL, FIX_ROTATION, FIX_POSITION or single bits); by default the tag with the most sightings is frozen wholly (the gauge)."""

    def __init__(self, rig=None, det=None, mounts=None, layout=None, fixed=None):
        from .apriltags import load_field_layout
        self.rig = rig
        self.det = rig.tasks[0].detector if rig is not None else det
        self.mounts = [_iso(m) for m in (mounts if mounts is not None else [t.robot_to_cam for t in rig.tasks])]
        if not 1 <= len(self.mounts) <= A.CK_RIG_MAX_CAMS:
            raise ValueError(f"a rig has 1..{A.CK_RIG_MAX_CAMS} cameras")
        self.field = None
        if layout is None:
            tags = rig.tasks[0].tags
        elif isinstance(layout, dict) and all(isinstance(v, A.Iso3) for v in layout.values()):
            tags = layout
        else:
            d = layout if isinstance(layout, dict) else json.load(open(layout))
            tags, self.field = load_field_layout(d), d.get("field")
        self.ids = sorted(tags)
        self.layout0 = [tags[i] for i in self.ids]
        self._by_pose = {}
        for k, iso in enumerate(self.layout0):
            if self._by_pose.setdefault(bytes(iso), k) != k:
                raise ValueError(f"tags {self.ids[self._by_pose[bytes(iso)]]} and {self.ids[k]} of the layout have the same pose: their sightings cannot be told apart")
        self.fixed = None if fixed is None else {int(k): int(v) for k, v in fixed.items()}
        self._steps, self._gyro = [], []

    def process(self, frames_per_camera, gyro):
        """rig.process_batch on frames_per_camera[c] = camera c's frames [n][h][w] with the headings gyro[n], then the steps of the
        call are appended from what it left on the device (ck_last_pose_inputs).  That call returns the tags' poses, not their ids:
        each is matched byte for byte against the layout the tasks were given.  An instant without a heading has no pose inputs and
        is not kept.  Returns rig.process_batch's result."""
        out = self.rig.process_batch(frames_per_camera, gyro)
        n = len(frames_per_camera[0])
        if n:
            per_cam = [last_pose_inputs(t.detector, n)[0] for t in self.rig.tasks]
            heading = [gyro if (gyro is None or np.isscalar(gyro)) else gyro[s] for s in range(n)]
            keep = [s for s in range(n) if heading[s] is not None]
            steps = []
            for s in keep:
                cams = []
                for c in range(len(per_cam)):
                    tags, bear = per_cam[c][s]
                    try:
                        cams.append(([self.ids[self._by_pose[bytes(t)]] for t in tags], bear))
                    except KeyError:
                        raise ValueError("a tag the detector solved with is not in the calibrator's layout") from None
                steps.append(cams)
            self.add_steps(steps, [heading[s] for s in keep])
        return out

    def add_steps(self, steps, gyro):
        """steps[s][c] = (tag ids [k], bearings (4 * k, 3)) of camera c; gyro[s] = the heading of the step (the rig solver's start
        needs it).  Returns the number of steps kept so far."""
        where = {tid: k for k, tid in enumerate(self.ids)}
        for cams, g in zip(steps, gyro):
            if len(cams) != len(self.mounts):
                raise ValueError("every step needs one entry per camera")
            self._steps.append([([where[int(t)] for t in ids], np.asarray(b, np.float64).reshape(-1, 3)) for ids, b in cams])
            self._gyro.append(float(g))
        return len(self._steps)

    def observations(self):
        """steps[s][c] = (tag ids, bearings) as add_steps takes them"""
        return [[([self.ids[k] for k in idx], b) for idx, b in cams] for cams in self._steps]

    def clear(self):
        self._steps, self._gyro = [], []

    def fixed6(self, fixed=None):
        """The mask of every layout entry: `fixed` ({tag id: mask}), the constructor's, or the most-sighted tag frozen wholly."""
        fixed = self.fixed if fixed is None else {int(k): int(v) for k, v in fixed.items()}
        fx = np.zeros(len(self.ids), np.uint8)
        if fixed is None:
            count = np.zeros(len(self.ids), np.int64)
            for cams in self._steps:
                for idx, _ in cams:
                    np.add.at(count, idx, 1)
            fx[int(np.argmax(count))] = FIX_ALL
        else:
            for tid, m in fixed.items():
                fx[self.ids.index(tid)] = m
        return fx

    def calibrate(self, fixed=None, leave_out=0, seed=0, max_iters=None):
        """Solves the kept steps (ck_field_calibrate_batch): a report dict, or None when the solve neither converged nor stalled at a
        finite rms.  report: results (the records of all problems), status, iters, rms, n_steps_used, poses, layout (the field.json
        dict of the solved layout: write it out and load it wherever the nominal one is loaded), tags ({id: {sightings, rms, moved:
        (metres, radians) from the nominal pose}}) and with leave_out = K > 0 per tag `std` (metres, radians): the spread of the
        solved pose over K random half-subsets (those that solved: `n_subsets`), all problems in the same device call."""
        p = params(max_iters)
        n_steps = len(self._steps)
        if n_steps < p.min_steps:
            return None
        problems, rng = [list(range(n_steps))], np.random.default_rng(seed)
        half = max(p.min_steps, (n_steps + 1) // 2)
        for _ in range(int(leave_out)):
            problems.append(sorted(rng.choice(n_steps, half, replace=False).tolist()))
        cap = Capture(self._steps, problems)
        res, lay, sight, rms, poses = calibrate_batch(self.det, p, cap, self.mounts, self.layout0, self.fixed6(fixed), self._gyro)
        ok = lambda r: r["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED) and np.isfinite(r["rms"])
        if not ok(res[0]):
            return None
        tags = {tid: {"sightings": int(sight[0][k]), "rms": float(rms[0][k]), "moved": tag_distance(self.layout0[k], lay[0][k])}
                for k, tid in enumerate(self.ids)}
        report = {"results": res, "status": STATUS_NAMES[int(res[0]["status"])], "iters": int(res[0]["iters"]), "rms": float(res[0]["rms"]),
                  "n_steps_used": int(res[0]["n_steps_used"]), "poses": poses[0], "layout": layout_dict(self.ids, lay[0], self.field), "tags": tags}
        if leave_out:
            sub = [i for i in range(1, len(res)) if ok(res[i])]
            report["n_subsets"] = len(sub)
            for k, tid in enumerate(self.ids):
                seen = [i for i in sub if sight[i][k] > 0]
                if len(seen) > 1:
                    t = np.array([lay[i][k]["t"] for i in seen])
                    ang = np.array([tag_distance(lay[0][k], lay[i][k])[1] for i in seen])
                    tags[tid]["std"] = (float(np.sqrt(np.sum(np.var(t, axis=0)))), float(np.sqrt(np.mean(ang ** 2))))
                else:
                    tags[tid]["std"] = None
        return report
