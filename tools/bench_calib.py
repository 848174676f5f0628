#!/usr/bin/env python3
"""Times ck_calib_refine_batch against ck_calib_refine_host looping the same problems on one thread in the same process:
a capture of 40 frames x 144 corners (the 6x6 board, 0.1 px noise) as one problem (B = 1, F = 40), one random half-subset (B = 1,
F = 20) and 64 random half-subsets in one call (B = 64).  Wall-clock per call, copies included; medians after warm-up.  One JSON line.

  python tools/bench_calib.py [--reps 15] [--warmup 3] [--subsets 64]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd import calibration as K  # noqa: E402
from chalkydri_amd._lib import check, lib  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector, _bind  # noqa: E402

W, H = 1600, 1304
CAM = np.array([1368.3343056383071, 1368.513346806007, 784.1021700594862, 655.1967162171935, -0.03428799012079279, -0.0021223103005884106,
                -0.001, -0.00014085919680638913, 0.015316405591806586])


def _rot(axis, angle):
    n = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def capture(n_frames, seed=0):
    rng = np.random.default_rng(seed)
    XY = K.Board.default_6x6().points()
    frames = []
    for _ in range(n_frames):
        a = rng.uniform(0, 2 * np.pi)
        R = _rot([np.cos(a), np.sin(a), 0], rng.uniform(0.15, 0.5)) @ _rot([0, 0, 1], rng.uniform(0, 2 * np.pi))
        t = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(1.1, 1.3)]) - R[:, :2] @ XY.mean(0)
        frames.append((XY, K.project(CAM, np.r_[R.ravel(), t], XY) + rng.normal(0, 0.1, XY.shape)))
    return frames


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--subsets", type=int, default=64)
    a = ap.parse_args()
    L = _bind(lib())
    det = AprilTagDetector(640, 480)
    frames = capture(40)
    rng = np.random.default_rng(1)
    halves = [[frames[i] for i in sorted(rng.choice(40, 20, replace=False))] for _ in range(a.subsets)]
    p = K.params(W, H)
    out = {"frames": 40, "points_per_frame": 144, "reps": a.reps, "warmup": a.warmup}
    for name, problems in (("full_B1_F40", [frames]), ("half_B1_F20", halves[:1]), ("half_B%d_F20" % a.subsets, halves)):
        pk = K.Packed(problems)
        starts = [K.calib_init(p, fr) for fr in problems]
        cams = (A.OpenCV5 * pk.n)(*[K._cam(s[0]) for s in starts])
        poses0 = np.ascontiguousarray(np.concatenate([s[1] for s in starts]))
        res_d, res_h = np.zeros(pk.n, K.RESULT_DTYPE), np.zeros(pk.n, K.RESULT_DTYPE)
        out_d, out_h = np.zeros((pk.n_frames, 12)), np.zeros((pk.n_frames, 12))
        rp = lambda r, i=0: C.cast(r.ctypes.data + i * K.RESULT_DTYPE.itemsize, C.POINTER(A.CalibResult))

        def device():
            check(L.ck_calib_refine_batch(det._h, C.byref(p), pk.prob, pk.n, *pk.args(), cams, poses0.ctypes.data, rp(res_d), out_d.ctypes.data), "ck_calib_refine_batch")

        def host():
            for i in range(pk.n):
                check(L.ck_calib_refine_host(C.byref(p), C.byref(pk.prob[i]), *pk.args(), C.byref(cams[i]), poses0.ctypes.data, rp(res_h, i), out_h.ctypes.data),
                      "ck_calib_refine_host")

        d, h = timed(device, a.reps, a.warmup), timed(host, max(3, a.reps // 3), 1)
        out[name] = {"device": d, "host_one_thread": h, "host_over_device": h["median_ms"] / d["median_ms"],
                     "same_bytes": bool(res_d.tobytes() == res_h.tobytes() and out_d.tobytes() == out_h.tobytes()),
                     "iters": [int(v) for v in res_d["iters"][:8]], "status": [int(v) for v in res_d["status"][:8]]}
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
