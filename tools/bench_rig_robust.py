#!/usr/bin/env python3
"""Times the robust rig solve beside the plain one on the same inputs: 256 instants x 3 cameras x 4 tags (np_rig.make_rig,
bearing noise 1e-3), (i) clean and (ii) with one wrong-id tag in every instant; ck_rig_solve_batch against ck_rig_solve_robust_batch,
synchronous calls on packed inputs (the C call alone is timed: copies in, kernel, records out), --warmup warm-ups and the median of
--reps calls each, and the mean number of GNC rounds of (ii).  One JSON line.

  python tools/bench_rig_robust.py [--reps 50] [--warmup 5] [--steps 256]
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
import np_rig_robust as NR  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd._lib import check  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402
from chalkydri_amd.rig import RESULT_DTYPE, ROBUST_RESULT_DTYPE, RigSolver, pack_steps  # noqa: E402
from chalkydri_amd.sqpnp import iso3  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def to_step(cams):
    return [([iso3(t, N.mat_to_quat(R)) for R, t in tags], b, iso3(bb, N.mat_to_quat(Am))) for tags, b, (Am, bb) in cams]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    clean, poisoned, gyros = [], [], []
    for _ in range(a.steps):
        c = NR.make_case(rng, 3, (4, 4), [(int(rng.integers(3)), int(rng.integers(4)), "id")])
        clean.append(to_step(c["clean"])); poisoned.append(to_step(c["cams"])); gyros.append(c["gyro"])
    det = AprilTagDetector(64, 64)
    L = det._L
    prm = RigSolver().params
    rprm = A.RigRobustParams()
    L.ck_rig_robust_params_default(C.byref(rprm))
    g = np.array(gyros)
    out = {"steps": a.steps, "cameras": 3, "tags_per_camera": 4, "reps": a.reps, "warmup": a.warmup}
    for name, steps in (("clean", clean), ("one_wrong_id", poisoned)):
        n_cams, probs, tarr, nt, barr = pack_steps(steps)
        res, rres = np.zeros(a.steps, RESULT_DTYPE), np.zeros(a.steps, ROBUST_RESULT_DTYPE)
        plain = timed(lambda: check(L.ck_rig_solve_batch(det._h, C.byref(prm), n_cams, probs, a.steps, tarr, nt, barr.ctypes.data, len(barr),
                                                         g.ctypes.data, res.ctypes.data_as(C.POINTER(A.RigResult))), "ck_rig_solve_batch"),
                      a.reps, a.warmup)
        robust = timed(lambda: check(L.ck_rig_solve_robust_batch(det._h, C.byref(rprm), n_cams, probs, a.steps, tarr, nt, barr.ctypes.data,
                                                                 len(barr), g.ctypes.data, rres.ctypes.data_as(C.POINTER(A.RigRobustResult))),
                                     "ck_rig_solve_robust_batch"), a.reps, a.warmup)
        out[name] = {"plain_median_ms": plain, "robust_median_ms": robust, "robust_over_plain": robust / plain,
                     "mean_rounds": float(rres["rounds"].mean()), "rejected_per_step": float(rres["n_rejected"].mean()),
                     "valid": int(rres["fused"]["valid"].sum())}
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
