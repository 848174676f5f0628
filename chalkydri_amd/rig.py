"""All the cameras of a robot fused into one robot pose: SQPnP over rays with different origins.

RigSolver is the stand-alone solver over the C ABI (ck_rig_solve_batch on a handle's device, ck_rig_solve_host without one);
AprilTagsRig runs one AprilTags task per camera and fuses what they left on the device (ck_rig_process_last).  Both take
`robust`: the solve that drops a wrong tag, GNC-TLS around the same solver (ck_rig_*_robust*), and `refine`
(DESIGN.md §4o): the maximum-likelihood pose behind either solve with the covariance of its own Jacobian (ck_rig_refine_*,
ck_rig_process_last_refined).
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._lib import check, lib
from .detector import _bind

RESULT_DTYPE = np.dtype([("valid", np.int32), ("n_tags", np.int32), ("rot", np.float64, (3, 3)), ("pos", np.float64, 3),
                         ("std_devs", np.float64, 3), ("yaw", np.float64), ("energy", np.float64),
                         ("cam_tags", np.int32, A.CK_RIG_MAX_CAMS), ("cam_rms", np.float64, A.CK_RIG_MAX_CAMS)])
assert RESULT_DTYPE.itemsize == C.sizeof(A.RigResult)
ROBUST_RESULT_DTYPE = np.dtype([("fused", RESULT_DTYPE), ("status", np.int32), ("rounds", np.int32), ("n_rejected", np.int32),
                                ("pad", np.int32), ("rejected", np.uint64, A.CK_RIG_MAX_CAMS), ("worst_inlier_rad", np.float64),
                                ("best_rejected_rad", np.float64)])
assert ROBUST_RESULT_DTYPE.itemsize == C.sizeof(A.RigRobustResult)
REFINED_DTYPE = np.dtype([("status", np.int32), ("iters", np.int32), ("n_points", np.int32), ("dof", np.int32), ("rot", np.float64, (3, 3)),
                          ("pos", np.float64, 3), ("cov", np.float64, (6, 6)), ("std_devs", np.float64, 3), ("cost0", np.float64),
                          ("cost", np.float64), ("rms", np.float64), ("chi2", np.float64), ("moved_m", np.float64),
                          ("moved_rad", np.float64), ("cam_rms", np.float64, A.CK_RIG_MAX_CAMS)])
assert REFINED_DTYPE.itemsize == C.sizeof(A.RigRefined)


class RobustParams:
    """gate_rad: the angle (rad) beyond which a tag's corners do not belong to the pose; mu_factor, max_rounds: the GNC schedule;
    min_inlier_tags: fewer tags than this left is no pose (status NO_CONSENSUS)."""

    def __init__(self, gate_rad=None, mu_factor=None, max_rounds=None, min_inlier_tags=None):
        self.gate_rad, self.mu_factor, self.max_rounds, self.min_inlier_tags = gate_rad, mu_factor, max_rounds, min_inlier_tags

    def _c(self, L, rig):
        p = A.RigRobustParams()
        L.ck_rig_robust_params_default(C.byref(p))
        p.rig = rig
        for k in ("gate_rad", "mu_factor", "max_rounds", "min_inlier_tags"):
            if getattr(self, k) is not None:
                setattr(p, k, getattr(self, k))
        return p


class RefineParams:
    """The maximum-likelihood refinement of the fused pose.  planar: solve (x, y, yaw) of a robot that stands on the
    floor at height z instead of six degrees of freedom; sigma: the standard deviation of a bearing (rad, per component); gyro_sigma
    (rad) > 0: the heading counts as a measurement of that standard deviation; max_iters: 1..100."""

    def __init__(self, planar=False, sigma=None, gyro_sigma=None, z=None, max_iters=None):
        self.planar, self.sigma, self.gyro_sigma, self.z, self.max_iters = planar, sigma, gyro_sigma, z, max_iters

    def _c(self, L):
        p = A.RigRefineParams()
        L.ck_rig_refine_params_default(C.byref(p))
        p.mode = A.CK_RIG_REFINE_PLANAR if self.planar else A.CK_RIG_REFINE_FREE
        for k, f in (("sigma", "sigma_rad"), ("gyro_sigma", "gyro_sigma_rad"), ("z", "z"), ("max_iters", "max_iters")):
            if getattr(self, k) is not None:
                setattr(p, f, getattr(self, k))
        return p


def _refine(refine):
    if refine is None or isinstance(refine, RefineParams):
        return refine
    if refine is True:
        return RefineParams()
    raise TypeError("refine is None, True or a RefineParams")


def _robust(robust):
    if robust is None or isinstance(robust, RobustParams):
        return robust
    if robust is True:
        return RobustParams()
    raise TypeError("robust is None, True or a RobustParams")


def pack_steps(steps):
    """steps[s][c] = (tags [Iso3], bearings (4 * len(tags), 3), robot_to_cam Iso3) for camera c at step s, every step with the
    same cameras.  Returns (n_cams, problems [n_cams * n] camera-major, tags array, bearings (m, 3))."""
    n = len(steps)
    n_cams = len(steps[0]) if n else 1
    probs = (A.SqpnpProblem * max(n_cams * n, 1))()
    tags, bear, nb = [], [], 0
    for s, cams in enumerate(steps):
        if len(cams) != n_cams:
            raise ValueError("every step needs the same number of cameras")
        for c, (iso, p2, rtc) in enumerate(cams):
            p2 = np.asarray(p2, np.float64).reshape(-1, 3)
            p = probs[c * n + s]
            p.n_tags, p.n_bearings, p.tag_offset, p.bearing_offset, p.robot_to_cam = len(iso), len(p2), len(tags), nb, rtc
            tags.extend(iso)
            bear.append(p2)
            nb += len(p2)
    tarr = (A.Iso3 * max(len(tags), 1))(*tags)
    barr = np.ascontiguousarray(np.concatenate(bear) if bear else np.zeros((0, 3)), np.float64)
    return n_cams, probs, tarr, len(tags), barr


class RigSolver:
    def __init__(self, handle=None, rig_id=255):
        """`handle`: an AprilTagDetector whose device and stream solve_batch runs on; solve_host needs none."""
        self._L = _bind(lib())
        self._det = handle
        self.params = A.RigParams()
        self._L.ck_rig_params_default(C.byref(self.params))
        self.params.rig_id = rig_id

    def max_iter(self, n):
        self.params.sqpnp.max_iter = int(n)
        return self

    def tolerance(self, tol):
        self.params.sqpnp.tol_sq = float(tol) * float(tol)
        return self

    def _solve(self, steps, gyro, host, robust=None):
        robust = _robust(robust)
        n = len(steps)
        n_cams, probs, tarr, nt, barr = pack_steps(steps)
        g = np.ascontiguousarray(gyro, np.float64).reshape(-1)
        if len(g) != n:
            raise ValueError("one gyro heading per step")
        g = g if n else np.zeros(1)
        if robust is not None:
            prm = robust._c(self._L, self.params)
            res = np.zeros(max(n, 1), ROBUST_RESULT_DTYPE)
            rp = res.ctypes.data_as(C.POINTER(A.RigRobustResult))
            if host:
                check(self._L.ck_rig_solve_robust_host(C.byref(prm), n_cams, probs, n, tarr, nt, barr.ctypes.data, len(barr),
                                                       g.ctypes.data, rp), "ck_rig_solve_robust_host")
            else:
                if self._det is None:
                    raise RuntimeError("RigSolver.solve_batch needs a device handle (pass an AprilTagDetector)")
                check(self._L.ck_rig_solve_robust_batch(self._det._h, C.byref(prm), n_cams, probs, n, tarr, nt, barr.ctypes.data,
                                                        len(barr), g.ctypes.data, rp), "ck_rig_solve_robust_batch")
            return res[:n]
        res = np.zeros(max(n, 1), RESULT_DTYPE)
        rp = res.ctypes.data_as(C.POINTER(A.RigResult))
        if host:
            check(self._L.ck_rig_solve_host(C.byref(self.params), n_cams, probs, n, tarr, nt, barr.ctypes.data, len(barr),
                                            g.ctypes.data, rp), "ck_rig_solve_host")
        else:
            if self._det is None:
                raise RuntimeError("RigSolver.solve_batch needs a device handle (pass an AprilTagDetector)")
            check(self._L.ck_rig_solve_batch(self._det._h, C.byref(self.params), n_cams, probs, n, tarr, nt, barr.ctypes.data,
                                             len(barr), g.ctypes.data, rp), "ck_rig_solve_batch")
        return res[:n]

    def solve_batch(self, steps, gyro, robust=None, refine=None):
        """One robot pose per step on the device; steps as pack_steps takes them.  Returns a RESULT_DTYPE array; with `robust` (True or
        a RobustParams) the solve that drops wrong tags and a ROBUST_RESULT_DTYPE array, the pose in its "fused".  With `refine` (True
        or a RefineParams) returns (those records, the REFINED_DTYPE records of refine_batch from them)."""
        res = self._solve(steps, gyro, False, robust)
        return res if refine is None else (res, self.refine_batch(steps, gyro, res, refine))

    def solve_host(self, steps, gyro, robust=None, refine=None):
        """The same on the host, one thread, no device."""
        res = self._solve(steps, gyro, True, robust)
        return res if refine is None else (res, self.refine_host(steps, gyro, res, refine))

    def _refine_call(self, steps, gyro, start, refine, host):
        refine = _refine(refine if refine is not None else True)
        n = len(steps)
        n_cams, probs, tarr, nt, barr = pack_steps(steps)
        prm = refine._c(self._L)
        g = None
        if gyro is not None:
            g = np.ascontiguousarray(gyro, np.float64).reshape(-1)
            if len(g) != n:
                raise ValueError("one gyro heading per step")
            g = g if n else np.zeros(1)
        start = np.asarray(start)
        rej = None
        if start.dtype == ROBUST_RESULT_DTYPE:
            rej = np.ascontiguousarray(start["rejected"])
            start = start["fused"]
        if start.dtype != RESULT_DTYPE or len(start) != n:
            raise ValueError("start: one fused record (RESULT_DTYPE or ROBUST_RESULT_DTYPE) per step")
        st = np.zeros(max(n, 1), RESULT_DTYPE)
        st[:n] = start
        out = np.zeros(max(n, 1), REFINED_DTYPE)
        args = [C.byref(prm), n_cams, probs, n, tarr, nt, barr.ctypes.data, len(barr), None if g is None else g.ctypes.data,
                st.ctypes.data, None if rej is None or n == 0 else rej.ctypes.data, out.ctypes.data_as(C.POINTER(A.RigRefined))]
        if host:
            check(self._L.ck_rig_refine_host(*args), "ck_rig_refine_host")
        else:
            if self._det is None:
                raise RuntimeError("RigSolver.refine_batch needs a device handle (pass an AprilTagDetector)")
            check(self._L.ck_rig_refine_batch(self._det._h, *args), "ck_rig_refine_batch")
        return out[:n]

    def refine_batch(self, steps, gyro, start, refine=True):
        """The maximum-likelihood pose and its covariance per step on the device, from the fused records `start` (what solve_batch
        returned for the same steps; a robust solve's records bring their rejection masks).  gyro may be None without a heading prior.
        Returns a REFINED_DTYPE array."""
        return self._refine_call(steps, gyro, start, refine, False)

    def refine_host(self, steps, gyro, start, refine=True):
        """The same on the host, one thread, no device: the kernel's twin."""
        return self._refine_call(steps, gyro, start, refine, True)


class AprilTagsRig:
    def __init__(self, tasks, rig_id=255, robust=None, refine=None):
        """tasks: one AprilTags task per camera (1..8, all on one device); sizes, calibrations and mounts may differ.  robust: True
        or a RobustParams for the solve that drops wrong tags (last_results is then of ROBUST_RESULT_DTYPE).  refine: True or a
        RefineParams, e.g. RefineParams(planar=True, gyro_sigma=0.01): the published measurement is the refined pose with the standard
        deviations of its covariance, and last_refined keeps the REFINED_DTYPE records beside last_results."""
        self.robust = _robust(robust)
        self.refine = _refine(refine)
        self.last_refined = None
        if not 1 <= len(tasks) <= A.CK_RIG_MAX_CAMS:
            raise ValueError(f"a rig has 1..{A.CK_RIG_MAX_CAMS} cameras")
        self.tasks = list(tasks)
        self.solver = RigSolver(self.tasks[0].detector, rig_id)
        self.solver.params.sqpnp = self.tasks[0]._pp.sqpnp
        self.solver.params.sign_change_error = self.tasks[0]._pp.sign_change_error

    def process_batch(self, frames_per_camera, gyro):
        """frames_per_camera[c] = camera c's frames [n][h][w], one per step; gyro: per-step heading or None entries.  Runs every
        task's process_batch, then fuses on the device.  Returns (rig records [n] of VisionMeasurement, rig valid flags,
        per-camera (records, valid) list); `last_results` keeps the RESULT_DTYPE records of the call.  With `refine` the rig records
        carry the refined pose and its standard deviations where the refinement has one, and `last_refined` keeps the REFINED_DTYPE
        records beside the fused ones."""
        if len(frames_per_camera) != len(self.tasks):
            raise ValueError("one frame batch per camera")
        n = len(frames_per_camera[0])
        per_cam = [t.process_batch(f, gyro) for t, f in zip(self.tasks, frames_per_camera)]
        dtype = RESULT_DTYPE if self.robust is None else ROBUST_RESULT_DTYPE
        if n == 0:
            self.last_results = np.zeros(0, dtype)
            self.last_refined = None if self.refine is None else np.zeros(0, REFINED_DTYPE)
            return (A.VisionMeasurement * 0)(), np.zeros(0, bool), per_cam
        g = np.zeros(max(n, 1), np.float64)
        has = np.zeros(max(n, 1), np.uint8)
        for i in range(n):
            gi = None if gyro is None else (gyro if np.isscalar(gyro) else gyro[i])
            if gi is not None:
                g[i], has[i] = gi, 1
        res = np.zeros(max(n, 1), dtype)
        meas = (A.VisionMeasurement * max(n, 1))()
        valid = (C.c_int32 * max(n, 1))()
        hs = (C.c_void_p * len(self.tasks))(*[t.detector._h.value for t in self.tasks])
        if self.refine is not None:
            prm = (self.robust or RobustParams())._c(self.solver._L, self.solver.params)
            fprm = self.refine._c(self.solver._L)
            refined = np.zeros(max(n, 1), REFINED_DTYPE)
            check(self.solver._L.ck_rig_process_last_refined(hs, len(self.tasks), n, C.byref(prm), int(self.robust is not None), C.byref(fprm),
                                                             g.ctypes.data, has.ctypes.data, res.ctypes.data,
                                                             refined.ctypes.data_as(C.POINTER(A.RigRefined)), meas, valid),
                  "ck_rig_process_last_refined")
            self.last_refined = refined[:n]
        elif self.robust is not None:
            prm = self.robust._c(self.solver._L, self.solver.params)
            check(self.solver._L.ck_rig_process_last_robust(hs, len(self.tasks), n, C.byref(prm), g.ctypes.data, has.ctypes.data,
                                                            res.ctypes.data_as(C.POINTER(A.RigRobustResult)), meas, valid),
                  "ck_rig_process_last_robust")
        else:
            check(self.solver._L.ck_rig_process_last(hs, len(self.tasks), n, C.byref(self.solver.params), g.ctypes.data, has.ctypes.data,
                                                     res.ctypes.data_as(C.POINTER(A.RigResult)), meas, valid), "ck_rig_process_last")
        self.last_results = res[:n]
        return (A.VisionMeasurement * n)(*meas[:n]), np.array(valid[:n], bool), per_cam
