"""Sub-pixel corners: the parameter records and the host twins of the device calls.

The device calls are methods of AprilTagDetector (corner_subpix, set_corner_subpix, board_corners); what is here needs no device:
the defaults, the weight table, and ck_corner_subpix_host / ck_board_corners_host, which return the bytes of the device calls."""
import ctypes as C

import numpy as np

from . import _abi as A
from ._lib import check, lib
from .detector import _bind, _images, _raw_detections

INFO_DTYPE = np.dtype([("status", "<i4"), ("iters", "<i4"), ("shift", "<f8")])
assert INFO_DTYPE.itemsize == C.sizeof(A.SubpixInfo)
STATUS_NAMES = {A.CK_SUBPIX_CONVERGED: "converged", A.CK_SUBPIX_MAXIT: "maxit", A.CK_SUBPIX_FLAT: "flat", A.CK_SUBPIX_REJECTED: "rejected"}


def subpix_params(half_win=None, max_iters=None, eps=None, det_min=None):
    """ck_subpix_params_t: the defaults (half_win 5, max_iters 30, eps 1e-3, det_min 1e-2) with the given fields replaced."""
    pp = A.SubpixParams()
    _bind(lib()).ck_subpix_params_default(C.byref(pp))
    for k, v in (("half_win", half_win), ("max_iters", max_iters)):
        if v is not None:
            setattr(pp, k, int(v))
    for k, v in (("eps", eps), ("det_min", det_min)):
        if v is not None:
            setattr(pp, k, float(v))
    return pp


def board_params(seed_max_shift=None, max_shift=None, probe=None, agree=None):
    """ck_board_params_t: the defaults (2.0, 2.5, (0.7, -0.6), 0.05 pixels) with the given fields replaced."""
    bp = A.BoardParams()
    _bind(lib()).ck_board_params_default(C.byref(bp))
    for k, v in (("seed_max_shift", seed_max_shift), ("max_shift", max_shift), ("agree", agree)):
        if v is not None:
            setattr(bp, k, float(v))
    if probe is not None:
        bp.probe[0], bp.probe[1] = float(probe[0]), float(probe[1])
    return bp


def board_desc(board, family=0):
    """ck_board_t of a calibration.Board."""
    return A.BoardDesc(int(board.rows), int(board.cols), int(board.first_id), int(family), float(board.tag_size), float(board.tag_spacing))


def weights(params=None):
    """ck_subpix_weights: the window's weight table [2w + 1][2w + 1]."""
    pp = params or subpix_params()
    side = 2 * pp.half_win + 1 if 2 <= pp.half_win <= 7 else 1
    out = np.zeros((side, side))
    check(_bind(lib()).ck_subpix_weights(C.byref(pp), out.ctypes.data), "ck_subpix_weights")
    return out


def corner_subpix_host(frames, frame, xy, params=None, return_info=False):
    """ck_corner_subpix_host: points xy [n][2] of frames [m][h][w] (or one [h][w]) refined on the host, one thread; frame: the
    frame of every point (an int or [n]).  The bytes of AprilTagDetector.corner_subpix."""
    pp = params or subpix_params()
    arr, keep = _images(frames)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    n = len(xy)
    fr = np.ascontiguousarray(np.broadcast_to(np.asarray(frame, np.int32), (n,)))
    out, info = np.empty((n, 2)), np.zeros(n, INFO_DTYPE)
    check(_bind(lib()).ck_corner_subpix_host(C.byref(pp), arr, len(arr), fr.ctypes.data, xy.ctypes.data, n, out.ctypes.data,
                                            info.ctypes.data), "ck_corner_subpix_host")
    return (out, info) if return_info else out


def board_corners_host(board, frames, dets, params=None, board_params_=None, family=0):
    """ck_board_corners_host: frames [n][h][w] and one list of detections per frame (Detection objects or ck_detection_t records)
    -> (uv [n][rows * cols][4][2], state [n][rows * cols]).  The bytes of AprilTagDetector.board_corners."""
    pp, bp, bd = params or subpix_params(), board_params_ or board_params(), board_desc(board, family)
    arr, keep = _images(frames)
    n = len(arr)
    if len(dets) != n:
        raise ValueError("one list of detections per frame")
    cap = max([len(d) for d in dets] + [1])
    da = (A.Detection * (n * cap))()
    counts = np.zeros(n, np.int32)
    for f, dl in enumerate(dets):
        one, k = _raw_detections(dl)
        counts[f] = k
        for i in range(k):
            da[f * cap + i] = one[i]
    nt = board.rows * board.cols
    uv, state, ntags = np.zeros((n, nt, 4, 2)), np.zeros((n, nt), np.uint8), np.zeros(n, np.int32)
    check(_bind(lib()).ck_board_corners_host(C.byref(bd), C.byref(pp), C.byref(bp), arr, n, da, cap, counts.ctypes.data, uv.ctypes.data,
                                            state.ctypes.data, ntags.ctypes.data), "ck_board_corners_host")
    return uv, state
