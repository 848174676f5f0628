"""Coloured game pieces: HSV mask, connected components, targets.

The device calls are methods of AprilTagDetector (detect_blobs, detect_blobs_device, blob_mask, blob_rgb) and of IngestRing
(detect_blobs); what is here needs no device: the parameter records, the tuning helper and the host twin (ck_blobs_host,
ck_blob_mask_host), which returns the bytes of the device calls given the pixels blob_rgb returns."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi as A
from ._lib import check, lib
from .detector import _bind

BLOB_DTYPE = np.dtype([("class_id", "<i4"), ("flags", "<i4"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                       ("seed", "<i4"), ("sx", "<i8"), ("sy", "<i8"), ("sxx", "<i8"), ("sxy", "<i8"), ("syy", "<i8"), ("cx", "<f8"),
                       ("cy", "<f8"), ("major", "<f8"), ("minor", "<f8"), ("axis", "<f8", 2), ("bearing", "<f8", 3), ("ground", "<f8", 2)])
assert BLOB_DTYPE.itemsize == C.sizeof(A.Blob)


@dataclass
class ColorClass:
    """One colour: 8-bit HSV bounds in OpenCV's ranges (h 0..179, s and v 0..255; h_min > h_max wraps through red) and the
    filter of its components.  max_area / max_aspect_permille 0: no upper bound.  ground_z: the plane the piece rests on."""
    h_min: int = 0
    h_max: int = 179
    s_min: int = 64
    s_max: int = 255
    v_min: int = 64
    v_max: int = 255
    min_area: int = 16
    max_area: int = 0
    min_fill_permille: int = 0
    min_aspect_permille: int = 0
    max_aspect_permille: int = 0
    ground_z: float = 0.0


def blob_params(classes=(ColorClass(),), erode=0, dilate=0, max_targets=16, max_components=4096, camera=None, robot_to_cam=None,
                max_range=20.0):
    """ck_blob_params_t.  camera: an A.Camera (chalkydri_amd.camera.camera_from_calib) for the bearings; robot_to_cam: an A.Iso3
    or (t [3], q [4] as w x y z), cam from robot as the solver takes it, for the ground points."""
    pp = A.BlobParams()
    _bind(lib()).ck_blob_params_default(C.byref(pp))
    classes = list(classes)
    if not 1 <= len(classes) <= A.CK_BLOB_MAX_CLASSES:
        raise ValueError(f"1..{A.CK_BLOB_MAX_CLASSES} classes")
    pp.n_classes, pp.erode, pp.dilate = len(classes), int(erode), int(dilate)
    pp.max_targets, pp.max_components, pp.max_range = int(max_targets), int(max_components), float(max_range)
    for i, c in enumerate(classes):
        k = pp.cls[i]
        for name in ("h_min", "h_max", "s_min", "s_max", "v_min", "v_max", "min_area", "max_area", "min_fill_permille",
                     "min_aspect_permille", "max_aspect_permille"):
            setattr(k, name, int(getattr(c, name)))
        k.ground_z = float(c.ground_z)
    if camera is not None:
        pp.has_camera, pp.cam = 1, camera
    if robot_to_cam is not None:
        pp.has_mount = 1
        if isinstance(robot_to_cam, A.Iso3):
            pp.robot_to_cam = robot_to_cam
        else:
            t, q = robot_to_cam
            for i in range(3):
                pp.robot_to_cam.t[i] = float(t[i])
            for i in range(4):
                pp.robot_to_cam.q[i] = float(q[i])
    return pp


def check_params(pp):
    """ck_blob_check: raises ChalkydriError (CK_EINVAL) for parameters out of range."""
    check(_bind(lib()).ck_blob_check(C.byref(pp)), "ck_blob_check")


def rgb_hsv(rgb):
    """ck_blob_rgb_hsv: uint8 [..., 3] RGB -> [..., 3] HSV by the library's integer definition."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    out = np.empty_like(rgb)
    check(_bind(lib()).ck_blob_rgb_hsv(rgb.ctypes.data, rgb.size // 3, out.ctypes.data), "ck_blob_rgb_hsv")
    return out


def _rgb_frames(rgb):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    if rgb.ndim == 3:
        rgb = rgb[None]
    if rgb.ndim != 4 or rgb.shape[3] != 3:
        raise ValueError("rgb is [n][H][W][3] uint8")
    return rgb


def mask_host(params, rgb, cls=0, stage=1):
    """ck_blob_mask_host: class cls's packed plane [n][H][ceil(W/32)] uint32 after the threshold (stage 0) or the morphology (1)."""
    rgb = _rgb_frames(rgb)
    n, H, W, _ = rgb.shape
    out = np.zeros((n, H, (W + 31) // 32), np.uint32)
    check(_bind(lib()).ck_blob_mask_host(C.byref(params), rgb.ctypes.data, W, H, n, int(cls), int(stage), out.ctypes.data), "ck_blob_mask_host")
    return out


def blobs_host(params, rgb, cap=None):
    """ck_blobs_host -> (records [n][n_classes][cap] as BLOB_DTYPE, counts [n][n_classes], status [n]).  cap: max_targets."""
    rgb = _rgb_frames(rgb)
    n, H, W, _ = rgb.shape
    cap = params.max_targets if cap is None else int(cap)
    out = np.zeros((n, params.n_classes, cap), BLOB_DTYPE)
    counts, status = np.zeros((n, params.n_classes), np.int32), np.zeros(n, np.uint32)
    buf = out if out.size else np.zeros(1, BLOB_DTYPE)
    check(_bind(lib()).ck_blobs_host(C.byref(params), rgb.ctypes.data, W, H, n, buf.ctypes.data, cap, counts.ctypes.data, status.ctypes.data),
          "ck_blobs_host")
    return out, counts, status


def unpack_mask(bits, width):
    """Packed planes [..., ceil(W/32)] uint32 -> bool [..., W]."""
    b = np.unpackbits(np.ascontiguousarray(bits, "<u4").view(np.uint8), axis=-1, bitorder="little")
    return b[..., :width].astype(bool)


def targets(records, counts, frame=0):
    """The written records of one frame, all classes, as a flat BLOB_DTYPE array (class by class, best first)."""
    cap = records.shape[2]
    rows = [records[frame, c, :min(int(counts[frame, c]), cap)] for c in range(records.shape[1])]
    return np.concatenate([r[r["area"] > 0] for r in rows])   # (a call truncated by max_targets leaves the rest zero)
