#!/usr/bin/env python3
"""Times the rig pose refinement beside the rig solve it follows, on the same inputs in the same run: 256 instants x 3
cameras x 4 tags (np_rig_refine.instant: a level robot, bearing noise 5e-4, heading noise 0.01 rad).  ck_rig_refine_time puts k_rig_refine
and k_rig between two events each, --reps times after --warmup; the medians are reported for both modes (six unknowns; planar with a
heading prior of 0.01 rad), with the mean number of iterations, and the one-thread twin's wall time for the same batch.  One JSON line.

  python tools/bench_rig_refine.py [--reps 50] [--warmup 5] [--steps 256]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import np_rig as N  # noqa: E402
import np_rig_refine as F  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd._lib import check  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402
from chalkydri_amd.rig import RefineParams, RigSolver, pack_steps  # noqa: E402
from chalkydri_amd.sqpnp import iso3  # noqa: E402


def to_step(cams):
    return [([iso3(t, N.mat_to_quat(R)) for R, t in tags], b, iso3(bb, N.mat_to_quat(Am))) for tags, b, (Am, bb) in cams]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    steps, gyros = [], []
    for _ in range(a.steps):
        steps.append(to_step(F.instant([4, 4, 4], rng))); gyros.append(F.TRUTH[2] + rng.normal(0, 0.01))
    det = AprilTagDetector(64, 64)
    L = det._L
    solver = RigSolver(det)
    g = np.array(gyros)
    n_cams, probs, tarr, nt, barr = pack_steps(steps)
    start = solver.solve_batch(steps, g)
    out = {"steps": a.steps, "cameras": 3, "tags_per_camera": 4, "reps": a.reps, "warmup": a.warmup, "valid": int(start["valid"].sum())}
    n = a.reps + a.warmup
    for name, rp in (("free", RefineParams(sigma=F.NOISE)), ("planar_prior", RefineParams(planar=True, sigma=F.NOISE, gyro_sigma=0.01, z=0.0))):
        prm = rp._c(L)
        ms_refine, ms_rig = np.zeros(n, np.float32), np.zeros(n, np.float32)
        check(L.ck_rig_refine_time(det._h, C.byref(prm), n_cams, probs, a.steps, tarr, nt, barr.ctypes.data, len(barr), g.ctypes.data, n,
                                   ms_refine.ctypes.data, ms_rig.ctypes.data), "ck_rig_refine_time")
        ref = solver.refine_batch(steps, g, start, rp)
        t = time.perf_counter()
        twin = solver.refine_host(steps, g, start, rp)
        host_ms = (time.perf_counter() - t) * 1e3
        k_refine, k_rig = float(np.median(ms_refine[a.warmup:])), float(np.median(ms_rig[a.warmup:]))
        out[name] = {"k_rig_refine_median_ms": k_refine, "k_rig_median_ms": k_rig, "refine_over_rig": k_refine / k_rig,
                     "mean_iters": float(ref["iters"].mean()), "maxiters": int((ref["status"] == A.CK_RIG_REFINE_MAXITERS).sum()),
                     "posed": int((ref["status"] <= A.CK_RIG_REFINE_MAXITERS).sum()), "twin_one_thread_ms": host_ms,
                     "device_equals_twin": ref.tobytes() == twin.tobytes()}
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
