#!/usr/bin/env python3
"""Times ck_fieldcal_refine_batch against ck_fieldcal_refine_host looping the same problems on one thread in the same
process: a capture of 3 cameras x 1000 steps in the room of the 32 tags of tests/golden/field.json at bearing noise 1e-3
(tests/np_fieldcal.py's generator), every tag but the gauge built up to 3 cm and 2 degrees away from the drawing, start poses from
ck_rig_solve_host with the drawing, as one problem (B = 1) and as 64 random half-subsets in one call (B = 64).  Wall-clock per call,
copies included; medians after warm-up.  One JSON line.

  python tools/bench_fieldcal.py [--steps 1000] [--reps 9] [--warmup 2] [--subsets 64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fieldcal_cases as FC  # noqa: E402
from chalkydri_amd import fieldcal as K  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402


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
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--subsets", type=int, default=64)
    a = ap.parse_args()
    cs = FC.acceptance_case(3, a.steps, 0, 1e-3, field=True)
    ok = cs["ok"]
    rng = np.random.default_rng(1)
    halves = [[ok[i] for i in sorted(rng.choice(len(ok), len(ok) // 2, replace=False))] for _ in range(a.subsets)]
    det = AprilTagDetector(640, 480)
    p = K.params()
    args = (cs["m_iso"], cs["lay0"], cs["fixed"], cs["poses0"])
    out = {"cameras": 3, "steps": a.steps, "steps_with_a_start": len(ok), "layout": len(cs["lay0"]), "reps": a.reps, "warmup": a.warmup}
    for name, problems in (("full_B1", [ok]), ("half_B%d" % a.subsets, halves)):
        cap = K.Capture(cs["steps"], problems)
        got = {}

        def device():
            got["d"] = K.refine_batch(det, p, cap, *args)

        def host():
            got["h"] = [K.refine_host(p, cap, *args, problem=i) for i in range(cap.n)]

        d, h = timed(device, a.reps, a.warmup), timed(host, max(2, a.reps // 4), 0)
        same = all(got["d"][j][i].tobytes() == got["h"][i][j].tobytes() for i in range(cap.n) for j in range(5))
        res, sight = got["d"][0], got["d"][2]
        out[name] = {"device": d, "host_one_thread": h, "host_over_device": h["median_ms"] / d["median_ms"], "same_bytes": bool(same),
                     "points": int(res[0]["n_points"]), "steps_used": int(res[0]["n_steps_used"]), "tags": int(np.sum(sight[0] > 0)),
                     "iters": [int(v) for v in res["iters"][:8]], "status": [int(v) for v in res["status"][:8]], "rms": float(res[0]["rms"])}
    det.close()
    print(json.dumps(out))
    if not all(v["same_bytes"] for v in out.values() if isinstance(v, dict)):
        sys.exit("device and host twin returned different bytes")


if __name__ == "__main__":
    main()
