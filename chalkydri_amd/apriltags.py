"""Host-side mirror of the `AprilTags` Copper sink task — the caller of the hot path
(crates/apriltags/src/lib.rs:166-182 struct, :221-291 new, :293-379 process) — batched over frames.

Configuration follows the reference: `family` (default tag36h11), `bits_corrected` (default 3), `cam_id`,
`robot_to_cam` JSON {roll,pitch,yaw,x,y,z} and `calib` JSON {"OpenCVModel5": {...}} (chalkydri.ron:28-29) or, for wide-angle
lenses, {"EUCM": {...}} / {"UCM": {...}} (chalkydri_amd/camera.py), and the field layout JSON (field.json; crates/apriltags/src/field_layout.rs:18-44).
"""
import ctypes as C
import json

import numpy as np

from . import _abi as A
from ._lib import check
from .detector import AprilTagDetector
from .sqpnp import SqPnP, iso3

SIGN_FLIP_CONST = 600.0  # crates/apriltags/src/lib.rs:6


def load_field_layout(path_or_dict):
    """field_layout.rs:18-44: id -> Isometry(translation, UnitQuaternion::from_quaternion(W,X,Y,Z)) (normalised)."""
    d = path_or_dict if isinstance(path_or_dict, dict) else json.load(open(path_or_dict))
    tags = {}
    for t in d["tags"]:
        tr, q = t["pose"]["translation"], t["pose"]["rotation"]["quaternion"]
        qq = np.array([q["W"], q["X"], q["Y"], q["Z"]], float)
        qq /= np.linalg.norm(qq)
        tags[int(t["ID"])] = iso3([tr["x"], tr["y"], tr["z"]], qq)
    return tags


class AprilTags:
    def __init__(self, width, height, field, calib, robot_to_cam, cam_id=0, family="tag36h11", bits_corrected=3,
                 max_batch=1, device=0, quad_sigma=0.0, fourcc=None, orientation="none", auto_exposure=False, exposure0=1.0,
                 exposure_params=None, jpeg_color=False, corner_subpix=None, blobs=None, planes=False, **cfg):
        """width x height is the image the detector sees, and calib its intrinsics: with an `orientation` ("none", "clockwise",
        "rotate-180", "counterclockwise": the reference's VideoOrientation names) those of the ORIENTED image.  `fourcc` names the
        raw format of the camera's frames for process_raw_batch ("YUYV", "RGB3", ...; None: 8-bit luma), or "MJPG" / "JPEG": the
        camera delivers one JPEG per frame (what the reference's USB cameras do at full rate), decoded and turned on the device;
        with jpeg_color=True the decode keeps the frames' chroma on the device, so that preview(color=True) works for them too.
        planes=True with "NV12" / "NV21" / "I420" / "YV12": the camera's frames carry their chroma planes behind the luma plane
        ([sh + ch][bytes] each), and preview(color=True) and `blobs` work for such a camera as for a packed colour format.
        auto_exposure=True (the reference's Camera.auto_exposure) meters the last frame of every batch the task stages, on the
        device, and keeps the exposure to set next in `exposure` (unit and start: exposure0); off, nothing is launched.
        corner_subpix=True (or a dict of AprilTagDetector.set_corner_subpix's arguments) refines every detection's corners to
        sub-pixel accuracy on the device before the pose is solved; off (the default), nothing is launched.
        blobs (a ck_blob_params_t from chalkydri_amd.blobs.blob_params, or a list of its ColorClass): the camera's second consumer,
        the reference's `ml` slot: after process_raw_batch of a packed colour format (or of JPEG frames with jpeg_color=True)
        `.blobs` holds the coloured targets of the frames just processed, found on the device in the same raw frames
        (AprilTagDetector.detect_blobs' triple), with the task's own calib and robot_to_cam behind the bearings and ground points."""
        if fourcc in A.JPEG_FOURCCS:
            from .detector import orientation_code
            orientation_code(orientation)                           # (ValueError for an unknown name, before any device work)
        calib = json.loads(calib) if isinstance(calib, str) else calib
        r2c = json.loads(robot_to_cam) if isinstance(robot_to_cam, str) else robot_to_cam
        from .camera import camera_from_calib
        self.camera = camera_from_calib(calib)                      # (ValueError for a model this library does not have)
        # the params' OpenCVModel5: the model itself, or (EUCM / UCM, set on the handle below, where this field is ignored) its pinhole part
        self.cam = A.OpenCV5(*([float(v) for v in self.camera.k] if self.camera.model == A.CK_CAMERA_OPENCV5 else
                               [float(v) for v in self.camera.k[:4]] + [0.0] * 5))
        # argument order of the reference call (lib.rs:247-254): x, y, z, roll, pitch, yaw
        self.robot_to_cam = SqPnP.create_solver_camera_transform(r2c["x"], r2c["y"], r2c["z"], r2c["roll"], r2c["pitch"], r2c["yaw"])
        self.detector = AprilTagDetector(width, height, max_batch=max_batch, families=(family,), bits_corrected=bits_corrected,
                                         device=device, quad_sigma=quad_sigma, corner_subpix=corner_subpix, **cfg)
        if self.camera.model != A.CK_CAMERA_OPENCV5:
            self.detector.set_camera(self.camera)
        self.solver = SqPnP(self.detector)
        self.tags = field if isinstance(field, dict) and all(isinstance(v, A.Iso3) for v in field.values()) else load_field_layout(field)
        self.cam_id = cam_id
        self.fourcc, self.orientation, self.jpeg_color = fourcc, orientation, bool(jpeg_color)
        self.planes = bool(planes)
        if self.planes and fourcc not in A.PLANAR_FOURCCS:
            raise ValueError(f"planes=True needs one of the planar formats {A.PLANAR_FOURCCS}")
        self._field = (A.FieldTag * max(len(self.tags), 1))()
        for i, (tid, pose) in enumerate(sorted(self.tags.items())):
            self._field[i].id, self._field[i].pose = tid, pose
        self._pp = A.ProcessParams()
        self._pp.cam, self._pp.robot_to_cam = self.cam, self.robot_to_cam
        self._pp.field, self._pp.n_field = self._field, len(self.tags)
        self._pp.camera_id, self._pp.sign_change_error = cam_id, SIGN_FLIP_CONST
        self._pp.sqpnp = self.solver._prm
        self.blobs, self._blob_params = None, None
        if blobs is not None:
            from .blobs import blob_params
            bp = blobs if isinstance(blobs, A.BlobParams) else blob_params(list(blobs))
            bp.has_camera, bp.cam, bp.has_mount, bp.robot_to_cam = 1, self.camera, 1, self.robot_to_cam
            self._blob_params = bp
        self._exposure = None
        if auto_exposure:
            from .exposure import ExposureController
            self._exposure = ExposureController(exposure_params, exposure0)

    def process_batch(self, frames=None, gyro=None, n=None):
        """frames [n][h][w] (or None to reuse uploaded frames); gyro: per-frame heading or None entries ("no gyro").
        Returns (records as a structured array of 64-byte VisionMeasurement, valid flags)."""
        det = self.detector
        if frames is not None:
            n = det.upload(frames)
        g = np.zeros(n, np.float64)
        has = np.zeros(n, np.uint8)
        for i in range(n):
            gi = None if gyro is None else (gyro if np.isscalar(gyro) else gyro[i])
            if gi is not None:
                g[i], has[i] = gi, 1
        out = (A.VisionMeasurement * n)()
        valid = (C.c_int32 * n)()
        check(det._L.ck_process_uploaded(det._h, n, C.byref(self._pp), g.ctypes.data, has.ctypes.data, out, valid), "ck_process_uploaded")
        if self._exposure is not None and n > 0:   # the newest frame of the batch says what to set for the next one
            self._exposure.update(det.exposure_stats(frames=[n - 1], params=self._exposure.params))
        return out, np.array(valid[:], bool)

    @property
    def exposure(self):
        """The exposure to set next, in exposure0's unit (None unless auto_exposure=True)."""
        return None if self._exposure is None else self._exposure.exposure

    def preview(self, frames=None, n=None, overlay=True, color=False, **kw):
        """After process_batch: the driver-station JPEGs (bytes each) of the frames just processed — indices into the staged
        frames, or n for 0..n-1 — scaled and encoded on the device, the tags the call found outlined (overlay=True).  Keyword
        arguments as AprilTagDetector.preview_jpeg (width=640, height=480, quality=50, restart_rows=0).  color=True: the colour
        files of the raw frames, after process_raw_batch of a packed colour format or of JPEG frames of a task made with
        jpeg_color=True (AprilTagDetector.preview_jpeg_color)."""
        call = self.detector.preview_jpeg_color if color else self.detector.preview_jpeg
        return call(frames, n, overlay=overlay, **kw)

    def process_raw_batch(self, raw_frames, gyro=None):
        """The camera's frames as it hands them over ([rows][bytes] each, in the task's fourcc): converted to luma and turned by
        the task's orientation on the device, then processed like process_batch."""
        if self.fourcc in A.JPEG_FOURCCS:   # one bytes object per frame
            n = self.detector.upload_jpeg(raw_frames, self.orientation, color=self.jpeg_color)
        else:
            n = self.detector.upload_raw(raw_frames, self.fourcc or "GREY", self.orientation, planes=self.planes)
        out = self.process_batch(None, gyro, n=n)
        if self._blob_params is not None:   # (a source without colour is an error here, not an empty answer)
            self.blobs = self.detector.detect_blobs(self._blob_params, n=n)
        return out

    process_raw = process_raw_batch

    def process_uploaded_into(self, n, gyro_ptr, has_gyro_ptr, out_ptr, valid_ptr):
        """Runs the whole path on the uploaded frames; every pointer may be host or device memory (no host round trip when
        the caller hands over device buffers, e.g. torch tensors that feed the RCCL pose gather)."""
        det = self.detector
        check(det._L.ck_process_uploaded(det._h, n, C.byref(self._pp), C.c_void_p(gyro_ptr), C.c_void_p(has_gyro_ptr),
                                         C.cast(C.c_void_p(out_ptr), C.POINTER(A.VisionMeasurement)),
                                         C.cast(C.c_void_p(valid_ptr), C.POINTER(C.c_int32))), "ck_process_uploaded")

    def process_device(self, ptr, n, stride, frame_pitch, gyro):
        det = self.detector
        g = np.ascontiguousarray(gyro, np.float64)
        has = np.ones(n, np.uint8)
        out = (A.VisionMeasurement * n)()
        valid = (C.c_int32 * n)()
        check(det._L.ck_process_batch_device(det._h, C.c_void_p(ptr), n, stride, frame_pitch, C.byref(self._pp), g.ctypes.data,
                                             has.ctypes.data, out, valid), "ck_process_batch_device")
        return out, np.array(valid[:], bool)


def measurements_to_bytes(records):
    """The exact datagram bytes whacknet would put on the wire (crates/whacknet/src/lib.rs:43-66,84-86)."""
    return [bytes(r) for r in records]
