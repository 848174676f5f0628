#!/usr/bin/env python3
"""Times the EUCM calibration: ck_camera_calibrate_batch, every problem from its six starts in one launch, against the
host twin looping the same starts on one thread (ck_camera_calib_init + ck_camera_calib_refine_host and the same selection rule) in
the same process.  A capture of 40 frames of the 6x6 board (0.1 px noise) through the wide lens of the tests (fx 500, alpha 0.62,
beta 1.08 on 1280 x 800): 64 random half-subsets in one call (64 x 6 = 384 problems in the launch) and one problem alone (6).
Wall-clock per call, starts and copies included; medians after warm-up.  One JSON line; numbers are recorded, not asserted.

  python tools/bench_camera_calib.py [--reps 9] [--warmup 2] [--subsets 64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd import calibration as K  # noqa: E402
from chalkydri_amd import camera  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402

W, H = 1280, 800
LENS = (500.0, 502.0, 640.0, 400.0, 0.62, 1.08)


def _rot(axis, angle):
    n = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def capture(n_frames, seed=0):
    rng = np.random.default_rng(seed)
    cam = camera.make_camera("EUCM", *LENS)
    XY = K.Board.default_6x6().points()
    frames = []
    while len(frames) < n_frames:
        a = rng.uniform(0, 2 * np.pi)
        R = _rot([np.cos(a), np.sin(a), 0], rng.uniform(0.1, 0.6)) @ _rot([0, 0, 1], rng.uniform(0, 2 * np.pi))
        ray, _ = camera.unproject_host(cam, [[rng.uniform(0.25 * W, 0.75 * W), rng.uniform(0.25 * H, 0.75 * H)]])
        t = rng.uniform(0.25, 0.6) * ray[0] - R[:, :2] @ XY.mean(0)
        uv, ok = camera.project(cam, XY @ R[:, :2].T + t)
        keep = ok & (uv[:, 0] >= 4) & (uv[:, 0] <= W - 5) & (uv[:, 1] >= 4) & (uv[:, 1] <= H - 5)
        if keep.sum() >= 24:
            frames.append((XY[keep], uv[keep] + rng.normal(0, 0.1, (int(keep.sum()), 2))))
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


def host_multi_start(p, frames):
    best = None
    for s in range(A.CK_CAMCAL_STARTS):
        k0, p0, _ = K.camera_calib_init("EUCM", p, frames, s)
        res, poses = K.camera_refine_host("EUCM", p, frames, k0, p0)
        if res["status"] != A.CK_CALIB_DEGENERATE and np.isfinite(res["cost"]) and (best is None or res["cost"] < best[0]["cost"]):
            res["start"], res["n_starts"] = s, A.CK_CAMCAL_STARTS
            best = (res, poses)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--subsets", type=int, default=64)
    a = ap.parse_args()
    det = AprilTagDetector(640, 480)
    frames = capture(40)
    rng = np.random.default_rng(1)
    halves = [[frames[i] for i in sorted(rng.choice(40, 20, replace=False))] for _ in range(a.subsets)]
    p = K.params(W, H)
    out = {"frames": 40, "points": int(sum(len(f[0]) for f in frames)), "starts": A.CK_CAMCAL_STARTS, "reps": a.reps, "warmup": a.warmup}
    for name, problems in (("half_B%d_F20" % a.subsets, halves), ("half_B1_F20", halves[:1]), ("full_B1_F40", [frames])):
        got = {}

        def device():
            got["d"] = K.camera_calibrate_batch(det, "EUCM", p, problems)

        def host():
            got["h"] = [host_multi_start(p, fr) for fr in problems]

        d, h = timed(device, a.reps, a.warmup), timed(host, max(2, a.reps // 4), 1)
        res = got["d"][0]
        same = all(hb is not None and hb[0].tobytes() == res[i].tobytes() and hb[1].tobytes() == got["d"][1][i].tobytes() for i, hb in enumerate(got["h"]))
        out[name] = {"device": d, "host_one_thread": h, "host_over_device": h["median_ms"] / d["median_ms"], "same_bytes": bool(same),
                     "winning_start": [int(v) for v in res["start"][:8]], "status": [int(v) for v in res["status"][:8]],
                     "rms": [round(float(v), 4) for v in res["rms"][:4]]}
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
