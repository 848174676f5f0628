"""Exposure metering: the loop the reference leaves open (`Camera.auto_exposure` / `manual_exposure`,
crates/chalkydri_core/src/config.rs:64-65; the V4L2 controls commented out in crates/chalkydri/src/cameras/pipeline.rs:237-245;
the stub crate crates/aaec).

Gradient-based metering with a gamma sweep (Shim, Lee and Kweon, 2014): the device histograms the Sobel gradient magnitude of
every staged frame under seven gamma curves (AprilTagDetector.exposure_stats); the host functions of the library turn a frame's
histograms into the gamma that carries the most gradient information and scale the caller's exposure by it.  Driving the camera
(V4L2, GStreamer) is the caller's part: the library only says what to set."""
import ctypes as C

import numpy as np

from . import _abi as A
from ._lib import check, lib

STATS_DTYPE = np.dtype([("luma", "<u4", (256,)), ("grad", "<u4", (A.CK_EXPOSURE_GAMMAS, A.CK_EXPOSURE_BINS)), ("n_luma", "<u4"),
                        ("n_grad", "<u4"), ("pad", "<u4", (2,))])
assert STATS_DTYPE.itemsize == C.sizeof(A.ExposureStats)


def _L():
    from .detector import _bind
    return _bind(lib())


class ExposureParams:
    """ck_exposure_params_t.  gamma: the seven curves, strictly increasing; lam, delta: the metric's weight; kp: gain of the
    recommendation; e_min, e_max: its clamp.  None keeps the library's default."""

    def __init__(self, gamma=None, lam=None, delta=None, kp=None, e_min=None, e_max=None):
        self.c = A.ExposureParams()
        _L().ck_exposure_params_default(C.byref(self.c))
        if gamma is not None:
            if len(gamma) != A.CK_EXPOSURE_GAMMAS:
                raise ValueError(f"gamma needs {A.CK_EXPOSURE_GAMMAS} values")
            for k, g in enumerate(gamma):
                self.c.gamma[k] = float(g)
        for name, v in (("lambda_", lam), ("delta", delta), ("kp", kp), ("e_min", e_min), ("e_max", e_max)):
            if v is not None:
                setattr(self.c, name, float(v))

    @property
    def gamma(self):
        return tuple(self.c.gamma)

    def luts(self):
        """[7][256] uint8: the tables the kernel maps a frame through (ck_exposure_luts).  No device needed."""
        out = np.empty((A.CK_EXPOSURE_GAMMAS, 256), np.uint8)
        check(_L().ck_exposure_luts(C.byref(self.c), out.ctypes.data), "ck_exposure_luts")
        return out


def _params(params):
    return params if isinstance(params, ExposureParams) else ExposureParams() if params is None else ExposureParams(**params)


def _record(stats):
    """One record of an exposure_stats result (or anything with its bytes) as a ctypes ck_exposure_stats_t."""
    a = np.ascontiguousarray(stats, STATS_DTYPE).reshape(-1)
    if a.size != 1:
        raise ValueError("one record is needed")
    return A.ExposureStats.from_buffer_copy(a.tobytes())


def metric(stats, params=None):
    """ck_exposure_metric: the gradient information of a frame under each of the seven curves."""
    p, s, m = _params(params), _record(stats), (C.c_double * A.CK_EXPOSURE_GAMMAS)()
    check(_L().ck_exposure_metric(C.byref(p.c), C.byref(s), m), "ck_exposure_metric")
    return list(m)


def recommend(stats, exposure, params=None):
    """ck_exposure_recommend: (the exposure to set next, gamma_hat).  gamma_hat < 1: the frame wants brightening."""
    p, s, nxt, g = _params(params), _record(stats), C.c_double(), C.c_double()
    check(_L().ck_exposure_recommend(C.byref(p.c), C.byref(s), float(exposure), C.byref(nxt), C.byref(g)), "ck_exposure_recommend")
    return nxt.value, g.value


def stats_call(det, ring_slot, n, frames, roi, params):
    """The one path of AprilTagDetector.exposure_stats and IngestRing.exposure_stats."""
    p = _params(params)
    if frames is None:
        if n is None:
            raise ValueError("frames (indices into the staged frames) or n is required")
        idx, n = None, int(n)
    else:
        idx = np.ascontiguousarray(frames, np.int32).reshape(-1)
        n = idx.size
    rects = None
    if roi is not None:
        r = np.asarray(roi, np.int64)
        r = np.broadcast_to(r, (n, 4)) if r.ndim == 1 else r
        if r.shape != (n, 4):
            raise ValueError("roi is one (x0, y0, x1, y1) or one per frame")
        rects = np.ascontiguousarray(np.clip(r, -2**31, 2**31 - 1), np.int32)
    out = np.zeros(max(n, 1), STATS_DTYPE)
    args = (idx.ctypes.data if idx is not None else None, n, C.byref(p.c), rects.ctypes.data if rects is not None else None, out.ctypes.data)
    if ring_slot is None:
        check(det._L.ck_exposure_stats(det._h, *args), "ck_exposure_stats")
    else:
        check(det._L.ck_exposure_stats_ingested(ring_slot[0], ring_slot[1], *args), "ck_exposure_stats_ingested")
    return out[:n]


def roi_from_detections(dets, margin, w, h):
    """The rectangle to meter next: the bounding box of a frame's detections (Detection objects) grown by `margin` pixels and
    clamped to the frame, or the whole frame when there are none."""
    if not dets:
        return 0, 0, w, h
    p = np.concatenate([np.asarray(d.corners(), float) for d in dets])
    c = lambda v, hi: int(min(max(v, 0), hi))
    return (c(np.floor(p[:, 0].min()) - margin, w), c(np.floor(p[:, 1].min()) - margin, h),
            c(np.floor(p[:, 0].max()) + 1 + margin, w), c(np.floor(p[:, 1].max()) + 1 + margin, h))


class ExposureController:
    """Keeps one camera's exposure, in the caller's unit (a V4L2 exposure_time_absolute, milliseconds, a gain), and moves it by
    what every metered frame recommends: update(stats) -> the exposure to set for the next frame."""

    def __init__(self, params=None, exposure0=1.0):
        self.params = _params(params)
        self.params.luts()                      # (refuses bad parameters here, not at the first frame)
        if not (np.isfinite(exposure0) and exposure0 > 0):
            raise ValueError("exposure0 must be positive")
        self.exposure, self.gamma_hat = float(exposure0), 1.0

    def update(self, stats):
        self.exposure, self.gamma_hat = recommend(stats, self.exposure, self.params)
        return self.exposure

    roi_from_detections = staticmethod(roi_from_detections)
