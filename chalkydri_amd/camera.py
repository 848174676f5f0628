"""Camera models: the reference's `calib` blob -> ck_camera_t, and pixel <-> bearing through the library.

The reference deserialises `calib` into camera_intrinsic_model::GenericModel<f64> (crates/apriltags/src/lib.rs:176,256), an enum by
model name.  Three of its models exist here:

    {"OpenCVModel5": {fx, fy, cx, cy, k1, k2, p1, p2, k3, width, height}}
    {"EUCM": {fx, fy, cx, cy, alpha, beta, width, height}}       the Enhanced Unified Camera Model (Khomutenko et al. 2016)
    {"UCM":  {fx, fy, cx, cy, alpha, width, height}}             = EUCM with beta = 1

(the EUCM / UCM field names by analogy with the OpenCVModel5 blob).  Any other key is a ValueError: KB4, EUCMT, FTheta
and the rational models need functions whose results differ between the host's and the device's maths libraries.
"""
import ctypes as C
import json

import numpy as np

from . import _abi as A
from ._lib import check, lib
from .detector import _bind

MODELS = {"OpenCVModel5": (A.CK_CAMERA_OPENCV5, ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")),
          "EUCM": (A.CK_CAMERA_EUCM, ("fx", "fy", "cx", "cy", "alpha", "beta")),
          "UCM": (A.CK_CAMERA_UCM, ("fx", "fy", "cx", "cy", "alpha"))}
NAMES = {code: name for name, (code, _) in MODELS.items()}


def make_camera(model, *k):
    """A.Camera of a model name (or code) and its parameters in ck_camera_t's order; checked (ValueError)."""
    code = MODELS[model][0] if isinstance(model, str) else int(model)
    cam = A.Camera()
    cam.model = code
    for i, v in enumerate(k):
        cam.k[i] = float(v)
    if code == A.CK_CAMERA_UCM:
        cam.k[5] = 1.0
    if _bind(lib()).ck_camera_check(C.byref(cam)) != A.CK_OK:
        raise ValueError(f"not a valid {NAMES.get(code, code)} camera: {list(cam.k)}")
    return cam


def camera_from_calib(blob):
    """The `calib` blob (dict or JSON text) -> A.Camera.  ValueError: not exactly one known model key, or parameters that
    ck_camera_check refuses; KeyError: a missing field."""
    blob = json.loads(blob) if isinstance(blob, str) else blob
    if isinstance(blob, A.Camera):
        return blob
    if not isinstance(blob, dict) or len(blob) != 1 or next(iter(blob)) not in MODELS:
        raise ValueError(f"calib must hold one of {sorted(MODELS)}, got {sorted(blob) if isinstance(blob, dict) else type(blob).__name__}")
    name, m = next(iter(blob.items()))
    return make_camera(name, *[m[f] for f in MODELS[name][1]])


def calib_from_camera(cam, width, height):
    """The blob of an A.Camera, in the schema camera_from_calib reads."""
    name = NAMES[cam.model]
    d = {f: float(cam.k[i]) for i, f in enumerate(MODELS[name][1])}
    d["width"], d["height"] = int(width), int(height)
    return {name: d}


def _call(fn, name, cam, pts, n_in, n_out):
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, n_in)
    out = np.empty((len(pts), n_out))
    ok = np.empty(len(pts), np.uint8)
    check(fn(C.byref(cam), pts.ctypes.data, len(pts), out.ctypes.data, ok.ctypes.data), name)
    return out, ok.astype(bool)


def unproject_host(cam, px):
    """Pixels [n][2] -> (unit bearings [n][3], ok [n]) on the host: the bytes of `unproject`."""
    return _call(_bind(lib()).ck_camera_unproject_host, "ck_camera_unproject_host", cam, px, 2, 3)


def unproject(cam, px):
    """Pixels [n][2] -> (unit bearings [n][3], ok [n]) on the device."""
    return _call(_bind(lib()).ck_camera_unproject, "ck_camera_unproject", cam, px, 2, 3)


def normalize_host(cam, px):
    """Pixels [n][2] -> (normalised points [n][2], ok [n]): what the per-tag pose works on (ok needs the ray in front of the camera)."""
    return _call(_bind(lib()).ck_camera_normalize_host, "ck_camera_normalize_host", cam, px, 2, 2)


def project(cam, xyz):
    """Camera points [n][3] -> (pixels [n][2], ok [n]); host arithmetic."""
    return _call(_bind(lib()).ck_camera_project_host, "ck_camera_project_host", cam, xyz, 3, 2)
