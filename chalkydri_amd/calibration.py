"""Camera calibration: host-side mirror of the reference configurator's `Calibrator` (crates/configurator/src/calibration.rs:30-143:
new, process, clear, calibrate) over the C ABI's ck_calib_* entry points.

The reference detects a 6x6 tag36h11 board, keeps a frame when at least MIN_CORNERS = 24 corners are seen and hands the frames to
an external solver.  Here `Calibrator.process` turns the detections of `detect_batch` into point correspondences and `calibrate`
solves them on the device: the intrinsics, one board pose per frame and, beyond the reference, the spread of every parameter over
random half-subsets of the capture, all problems in one batched call.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._lib import check, lib
from .detector import _bind

MIN_CORNERS = 24  # calibration.rs:30
PARAM_NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
STATUS_NAMES = {A.CK_CALIB_CONVERGED: "converged", A.CK_CALIB_STALLED: "stalled", A.CK_CALIB_MAXIT: "maxit",
                A.CK_CALIB_DEGENERATE: "degenerate"}
FIX_DISTORTION, FIX_FOCAL = A.CK_CALIB_FIX_DISTORTION, A.CK_CALIB_FIX_FOCAL
RESULT_DTYPE = np.dtype([("cam", "<f8", (9,)), ("status", "<i4"), ("iters", "<i4"), ("n_frames", "<i4"), ("n_points", "<i4"),
                         ("rms", "<f8"), ("cost0", "<f8"), ("cost", "<f8")])
assert RESULT_DTYPE.itemsize == C.sizeof(A.CalibResult)
# ck_camera_calib_result_t: any camera model (chalkydri_amd/camera.py); `cam` = ck_camera_t.k, `start` of `n_starts` = the winner
CAMERA_RESULT_DTYPE = np.dtype([("model", "<i4"), ("pad", "<i4"), ("cam", "<f8", (9,)), ("status", "<i4"), ("iters", "<i4"),
                                ("n_frames", "<i4"), ("n_points", "<i4"), ("rms", "<f8"), ("cost0", "<f8"), ("cost", "<f8"),
                                ("start", "<i4"), ("n_starts", "<i4")])
assert CAMERA_RESULT_DTYPE.itemsize == C.sizeof(A.CameraCalibResult)
MODEL_CODES = {"OpenCVModel5": A.CK_CAMERA_OPENCV5, "EUCM": A.CK_CAMERA_EUCM, "UCM": A.CK_CAMERA_UCM}


class Board:
    """A grid of tags on a plane: rows x cols tags of edge `tag_size` metres (the black square), `tag_spacing` times that between
    neighbours, ids row-major from the board's origin starting at first_id (the aprilgrid convention).  Board coordinates: x along
    a row, y along a column, the first tag's outer corner region starting at the origin; seen from the front x points right and y
    down, like the image, so a board pose has its z axis pointing away from the camera."""

    def __init__(self, rows=6, cols=6, tag_size=0.088, tag_spacing=0.3, first_id=0):
        if rows < 1 or cols < 1 or not tag_size > 0 or tag_spacing < 0:
            raise ValueError("a board has rows, cols >= 1, tag_size > 0 and tag_spacing >= 0")
        self.rows, self.cols, self.tag_size, self.tag_spacing, self.first_id = int(rows), int(cols), float(tag_size), float(tag_spacing), int(first_id)

    @classmethod
    def default_6x6(cls):
        """The board of the reference's `create_default_6x6_board()`.  Tag size 0.088 m and spacing ratio 0.3 are the defaults of the
        external camera-intrinsic-calibration crate that function belongs to, not values of the reference itself: measure the
        printed board and pass its own numbers to Board(...)."""
        return cls(6, 6, 0.088, 0.3, 0)

    @property
    def pitch(self):
        return self.tag_size * (1.0 + self.tag_spacing)

    def ids(self):
        return range(self.first_id, self.first_id + self.rows * self.cols)

    def tag_center(self, tag_id):
        k = tag_id - self.first_id
        if not 0 <= k < self.rows * self.cols:
            raise KeyError(tag_id)
        return np.array([(k % self.cols) * self.pitch + self.tag_size / 2, (k // self.cols) * self.pitch + self.tag_size / 2])

    def tag_corners(self, tag_id):
        """Board-plane coordinates [4][2] of the tag's corners in ck_detection_t's corner order: (-1, 1), (1, 1), (1, -1), (-1, -1)
        times half the tag size about the tag's centre."""
        s = self.tag_size / 2
        return self.tag_center(tag_id) + s * np.array([[-1.0, 1.0], [1.0, 1.0], [1.0, -1.0], [-1.0, -1.0]])

    def points(self):
        """All corners [rows * cols * 4][2], by id and corner."""
        return np.concatenate([self.tag_corners(i) for i in self.ids()])


def params(width, height, fixed_mask=0, max_iters=None, min_points_per_frame=None, min_frames=None):
    """ck_calib_params_t; None keeps the library's default (100 iterations, 24 points per frame, 3 frames)."""
    p = A.CalibParams()
    _bind(lib()).ck_calib_params_default(C.byref(p), int(width), int(height))
    p.fixed_mask = int(fixed_mask)
    for name, v in (("max_iters", max_iters), ("min_points_per_frame", min_points_per_frame), ("min_frames", min_frames)):
        if v is not None:
            setattr(p, name, int(v))
    return p


class Packed:
    """The shared arrays of a call: problems = a list of problems, each a list of frames (board_xy [n][2], image_uv [n][2])."""

    def __init__(self, problems):
        self.n = len(problems)
        self.prob = (A.CalibProblem * max(self.n, 1))()
        bxy, uv, starts, n_pts, n_frames = [], [], [], 0, 0
        for i, frames in enumerate(problems):
            self.prob[i].n_frames, self.prob[i].start_offset = len(frames), len(starts)
            self.prob[i].point_offset, self.prob[i].pose_offset = n_pts, n_frames
            at = 0
            starts.append(0)
            for b, u in frames:
                b, u = np.asarray(b, np.float64).reshape(-1, 2), np.asarray(u, np.float64).reshape(-1, 2)
                if len(b) != len(u):
                    raise ValueError("a frame has as many board points as image points")
                bxy.append(b)
                uv.append(u)
                at += len(b)
                starts.append(at)
            n_pts += at
            n_frames += len(frames)
        self.board_xy = np.ascontiguousarray(np.concatenate(bxy) if bxy else np.zeros((0, 2)), np.float64)
        self.image_uv = np.ascontiguousarray(np.concatenate(uv) if uv else np.zeros((0, 2)), np.float64)
        self.frame_start = np.array(starts, np.int32)
        self.n_points, self.n_starts, self.n_frames = n_pts, len(starts), n_frames

    def args(self):
        return (self.board_xy.ctypes.data, self.image_uv.ctypes.data, self.frame_start.ctypes.data, self.n_points, self.n_starts, self.n_frames)

    def poses_of(self, poses, i):
        q = self.prob[i]
        return poses[q.pose_offset:q.pose_offset + q.n_frames]


def _cam(k):
    return A.OpenCV5(*[float(v) for v in k])


def calib_init(p, frames):
    """ck_calib_init of one problem, on the host: (cam0 [9], poses0 [F][12], status)."""
    pk = Packed([frames])
    cam0, poses, st = A.OpenCV5(), np.zeros((pk.n_frames, 12)), C.c_int32(-1)
    check(_bind(lib()).ck_calib_init(C.byref(p), pk.prob, *pk.args(), C.byref(cam0), poses.ctypes.data, C.byref(st)), "ck_calib_init")
    return np.array([getattr(cam0, n) for n in PARAM_NAMES]), poses, st.value


def jacobian(cam, pose, board_xy, image_uv, fixed_mask=0):
    """ck_calib_jacobian: the solver's residuals [n][2] and analytic Jacobian [n][2][15] of one frame's observations."""
    b, u = np.ascontiguousarray(board_xy, np.float64).reshape(-1, 2), np.ascontiguousarray(image_uv, np.float64).reshape(-1, 2)
    pose = np.ascontiguousarray(pose, np.float64).reshape(12)
    r, J = np.zeros((len(b), 2)), np.zeros((len(b), 2, 15))
    check(_bind(lib()).ck_calib_jacobian(C.byref(_cam(cam)), pose.ctypes.data, b.ctypes.data, u.ctypes.data, len(b), int(fixed_mask),
                                         r.ctypes.data, J.ctypes.data), "ck_calib_jacobian")
    return r, J


def refine_host(p, frames, cam0, poses0):
    """ck_calib_refine_host of one problem, one host thread: (result record, poses [F][12])."""
    pk = Packed([frames])
    res, out = np.zeros((), RESULT_DTYPE), np.zeros((pk.n_frames, 12))
    poses0 = np.ascontiguousarray(poses0, np.float64).reshape(pk.n_frames, 12)
    check(_bind(lib()).ck_calib_refine_host(C.byref(p), pk.prob, *pk.args(), C.byref(_cam(cam0)), poses0.ctypes.data,
                                            C.cast(res.ctypes.data, C.POINTER(A.CalibResult)), out.ctypes.data), "ck_calib_refine_host")
    return res, out


def refine_batch(det, p, problems, cams0, poses0):
    """ck_calib_refine_batch on the detector's handle: problems as for Packed, cams0 [B][9], poses0 a list of [F_i][12].  Returns
    (result records [B], list of poses [F_i][12])."""
    pk = Packed(problems)
    cams = (A.OpenCV5 * max(pk.n, 1))(*[_cam(k) for k in cams0])
    pin = np.ascontiguousarray(np.concatenate([np.asarray(q, np.float64).reshape(-1, 12) for q in poses0]) if pk.n else np.zeros((0, 12)))
    res, out = np.zeros(pk.n, RESULT_DTYPE), np.zeros((pk.n_frames, 12))
    check(_bind(lib()).ck_calib_refine_batch(det._h, C.byref(p), pk.prob, pk.n, *pk.args(), cams, pin.ctypes.data,
                                             C.cast(res.ctypes.data, C.POINTER(A.CalibResult)), out.ctypes.data), "ck_calib_refine_batch")
    return res, [pk.poses_of(out, i).copy() for i in range(pk.n)]


def calibrate_batch(det, p, problems):
    """ck_calibrate_batch: the start on the host, the refinement of all problems in one launch."""
    pk = Packed(problems)
    res, out = np.zeros(pk.n, RESULT_DTYPE), np.zeros((pk.n_frames, 12))
    check(_bind(lib()).ck_calibrate_batch(det._h, C.byref(p), pk.prob, pk.n, *pk.args(), C.cast(res.ctypes.data, C.POINTER(A.CalibResult)),
                                          out.ctypes.data), "ck_calibrate_batch")
    return res, [pk.poses_of(out, i).copy() for i in range(pk.n)]


def _model(model):
    return MODEL_CODES[model] if isinstance(model, str) else int(model)


def _camera(model, k):
    cam = A.Camera()
    cam.model = _model(model)
    for i, v in enumerate(k):
        cam.k[i] = float(v)
    return cam


def _cres(arr):
    return C.cast(arr.ctypes.data, C.POINTER(A.CameraCalibResult))


def camera_calib_init(model, p, frames, start_index=0):
    """ck_camera_calib_init of one problem, on the host: start `start_index` of the model's starts -> (k0 [9], poses0 [F][12], status)."""
    pk = Packed([frames])
    cam0, poses, st = A.Camera(), np.zeros((pk.n_frames, 12)), C.c_int32(-1)
    check(_bind(lib()).ck_camera_calib_init(_model(model), C.byref(p), pk.prob, *pk.args(), int(start_index), C.byref(cam0), poses.ctypes.data,
                                            C.byref(st)), "ck_camera_calib_init")
    return np.array(cam0.k[:]), poses, st.value


def camera_jacobian(model, k, pose, board_xy, image_uv, fixed_mask=0):
    """ck_camera_calib_jacobian: residuals [n][2] and analytic Jacobian [n][2][15] of one frame's observations under `model`."""
    b, u = np.ascontiguousarray(board_xy, np.float64).reshape(-1, 2), np.ascontiguousarray(image_uv, np.float64).reshape(-1, 2)
    pose = np.ascontiguousarray(pose, np.float64).reshape(12)
    r, J = np.zeros((len(b), 2)), np.zeros((len(b), 2, 15))
    check(_bind(lib()).ck_camera_calib_jacobian(_model(model), C.byref(_camera(model, k)), pose.ctypes.data, b.ctypes.data, u.ctypes.data, len(b),
                                                int(fixed_mask), r.ctypes.data, J.ctypes.data), "ck_camera_calib_jacobian")
    return r, J


def camera_refine_host(model, p, frames, k0, poses0):
    """ck_camera_calib_refine_host of one problem, one host thread: (result record, poses [F][12])."""
    pk = Packed([frames])
    res, out = np.zeros((), CAMERA_RESULT_DTYPE), np.zeros((pk.n_frames, 12))
    poses0 = np.ascontiguousarray(poses0, np.float64).reshape(pk.n_frames, 12)
    check(_bind(lib()).ck_camera_calib_refine_host(_model(model), C.byref(p), pk.prob, *pk.args(), C.byref(_camera(model, k0)), poses0.ctypes.data,
                                                   _cres(res), out.ctypes.data), "ck_camera_calib_refine_host")
    return res, out


def camera_refine_batch(det, model, p, problems, cams0, poses0):
    """ck_camera_calib_refine_batch on the detector's handle: as refine_batch, for any model."""
    pk = Packed(problems)
    cams = (A.Camera * max(pk.n, 1))(*[_camera(model, k) for k in cams0])
    pin = np.ascontiguousarray(np.concatenate([np.asarray(q, np.float64).reshape(-1, 12) for q in poses0]) if pk.n else np.zeros((0, 12)))
    res, out = np.zeros(pk.n, CAMERA_RESULT_DTYPE), np.zeros((pk.n_frames, 12))
    check(_bind(lib()).ck_camera_calib_refine_batch(det._h, _model(model), C.byref(p), pk.prob, pk.n, *pk.args(), cams, pin.ctypes.data, _cres(res),
                                                    out.ctypes.data), "ck_camera_calib_refine_batch")
    return res, [pk.poses_of(out, i).copy() for i in range(pk.n)]


def camera_calibrate_batch(det, model, p, problems):
    """ck_camera_calibrate_batch: every problem from every start of its model in one launch, the lowest final cost kept."""
    pk = Packed(problems)
    res, out = np.zeros(pk.n, CAMERA_RESULT_DTYPE), np.zeros((pk.n_frames, 12))
    check(_bind(lib()).ck_camera_calibrate_batch(det._h, _model(model), C.byref(p), pk.prob, pk.n, *pk.args(), _cres(res), out.ctypes.data),
          "ck_camera_calibrate_batch")
    return res, [pk.poses_of(out, i).copy() for i in range(pk.n)]


def project(k, pose, board_xy, model="OpenCVModel5"):
    """The forward model on the host (numpy), for reports: k [9], pose [12] (R row-major, t), board_xy [n][2] -> pixels [n][2]."""
    R, t = np.asarray(pose[:9]).reshape(3, 3), np.asarray(pose[9:])
    P = np.asarray(board_xy) @ R[:, :2].T + t
    if _model(model) != A.CK_CAMERA_OPENCV5:
        d = np.sqrt(k[5] * (P[:, 0] ** 2 + P[:, 1] ** 2) + P[:, 2] ** 2)
        den = k[4] * d + (1 - k[4]) * P[:, 2]
        return np.stack([k[0] * P[:, 0] / den + k[2], k[1] * P[:, 1] / den + k[3]], 1)
    x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    r2 = x * x + y * y
    rad = 1 + r2 * (k[4] + r2 * (k[5] + r2 * k[8]))
    xd = x * rad + 2 * k[6] * x * y + k[7] * (r2 + 2 * x * x)
    yd = y * rad + k[6] * (r2 + 2 * y * y) + 2 * k[7] * x * y
    return np.stack([k[0] * xd + k[2], k[1] * yd + k[3]], 1)


class Calibrator:
    """Calibrator::{new, process, clear, calibrate} of the reference, with `det` an AprilTagDetector of the camera's geometry."""

    def __init__(self, det, board=None, min_corners=MIN_CORNERS, recover=False, subpix=None, board_params=None):
        """recover=True: `process` recovers the whole board from the tags that decoded (AprilTagDetector.board_corners: the tags'
        corners refined to sub-pixel accuracy, their neighbours predicted, refined and checked), which on an AprilGrid — black
        squares at the tags' corners — finds several times the tags at a third of the corner error; `subpix` (an A.SubpixParams)
        and `board_params` (an A.BoardParams) are its settings.  recover=False is the reference's path."""
        self.det, self.board, self.min_corners = det, board or Board.default_6x6(), int(min_corners)
        self.recover, self.subpix, self.board_params = bool(recover), subpix, board_params
        self._ids = set(self.board.ids())
        self._frames = []

    def process(self, frames):
        """Detects the board in frames [n][h][w] (or one [h][w]) and keeps every frame with at least min_corners corners of the
        board's ids decoded without a corrected bit; returns the number of frames kept so far, like the reference."""
        if self.recover:
            return self._process_recover(frames)
        for dets in self.det.detect_batch(frames, cap=max(64, len(self._ids))):
            seen, b, u = set(), [], []
            for d in dets:
                if d.id() in self._ids and d.hamming() == 0 and d.family() == 0 and d.id() not in seen:
                    seen.add(d.id())
                    b.append(self.board.tag_corners(d.id()))
                    u.append(d.corners())
            if 4 * len(seen) >= self.min_corners:
                self._frames.append((np.concatenate(b), np.concatenate(u)))
        return len(self._frames)

    def _process_recover(self, frames):
        frames = np.asarray(frames)
        frames = frames[None] if frames.ndim == 2 else frames
        ids = list(self.board.ids())
        for i0 in range(0, len(frames), self.det.max_batch):
            self.det.detect_batch(frames[i0:i0 + self.det.max_batch], cap=max(64, len(ids)))
            uv, state = self.det.board_corners(self.board, self.subpix, self.board_params)
            for f in range(len(uv)):
                known = np.nonzero(state[f])[0]
                if 4 * len(known) >= self.min_corners:
                    self._frames.append((np.concatenate([self.board.tag_corners(ids[t]) for t in known]), uv[f, known].reshape(-1, 2).copy()))
        return len(self._frames)

    def add_observations(self, board_xy, image_uv):
        """Keeps a frame of correspondences the caller found itself (board_xy [n][2] metres, image_uv [n][2] pixels), like
        chalkydri::Calibrator::add_observations; False (and nothing kept) below min_corners points."""
        b, u = np.asarray(board_xy, np.float64).reshape(-1, 2), np.asarray(image_uv, np.float64).reshape(-1, 2)
        if len(b) != len(u):
            raise ValueError("a frame has as many board points as image points")
        if len(b) < self.min_corners:
            return False
        self._frames.append((b.copy(), u.copy()))
        return True

    def observations(self):
        """The kept frames: a list of (board_xy [n][2], image_uv [n][2])."""
        return list(self._frames)

    def clear(self):
        self._frames = []

    def calibrate(self, fixed_mask=0, leave_out=0, seed=0, max_iters=None, model="OpenCVModel5"):
        """Solves the kept frames: (calib_dict, report), or None when the solve neither converged nor stalled at a finite rms (the
        reference likewise returns None after its retries).  calib_dict is what AprilTags(..., calib=) takes, in the schema of
        `model`: "OpenCVModel5", or "EUCM" / "UCM" for wide-angle lenses (every problem is then solved from six starts in the same
        launch and the lowest final cost kept: report["start"]; fixed_mask bits 0..5 = fx fy cx cy alpha beta).  report: status,
        iters, rms, per_frame_rms, poses, and with leave_out = K > 0 `std`, the standard deviation of each parameter over K
        random half-subsets of the frames (those that solved: `n_subsets`), all solved in the same batched call."""
        frames = self._frames
        p = params(self.det.width, self.det.height, fixed_mask, max_iters, max(4, self.min_corners))
        if len(frames) < p.min_frames:
            return None
        problems, rng = [frames], np.random.default_rng(seed)
        half = max(p.min_frames, (len(frames) + 1) // 2)
        for _ in range(int(leave_out)):
            problems.append([frames[i] for i in sorted(rng.choice(len(frames), half, replace=False))])
        if _model(model) == A.CK_CAMERA_OPENCV5:
            res, poses = calibrate_batch(self.det, p, problems)
        else:
            res, poses = camera_calibrate_batch(self.det, model, p, problems)
        ok = lambda r: r["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED) and np.isfinite(r["rms"])
        if not ok(res[0]):
            return None
        k = res[0]["cam"]
        if _model(model) == A.CK_CAMERA_OPENCV5:
            names = PARAM_NAMES
            calib = {"OpenCVModel5": dict({n: float(v) for n, v in zip(PARAM_NAMES, k)}, width=int(self.det.width), height=int(self.det.height))}
        else:
            from .camera import MODELS, calib_from_camera
            names = MODELS[model][1]
            calib = calib_from_camera(_camera(model, k), self.det.width, self.det.height)
        per_frame = [float(np.sqrt(np.mean(np.sum((project(k, P, b, model) - u) ** 2, 1)))) for (b, u), P in zip(frames, poses[0])]
        report = {"status": STATUS_NAMES[int(res[0]["status"])], "iters": int(res[0]["iters"]), "rms": float(res[0]["rms"]),
                  "per_frame_rms": per_frame, "poses": poses[0]}
        if _model(model) != A.CK_CAMERA_OPENCV5:
            report["start"], report["n_starts"] = int(res[0]["start"]), int(res[0]["n_starts"])
        if leave_out:
            sub = np.array([r["cam"] for r in res[1:] if ok(r)])
            report["n_subsets"] = len(sub)
            report["std"] = {n: float(v) for n, v in zip(names, sub.std(0))} if len(sub) > 1 else None
        return calib, report
