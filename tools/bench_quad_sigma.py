#!/usr/bin/env python3
"""quad_sigma cost on bench.py's workload (scenes.bench_stream(2, n, 1280, 800, 8 tags, noise_amp=3)): detect + pose per step and
frames/s for sigma in {0, 0.8, -0.8, 2.0} x quad_decimate in {1, 2} (steps timed between device events after warm-up), plus the
front end alone (ck_time_threshold_segment: filter + threshold + segmentation, and its difference to the unfiltered pass) and the
filtered images' effect on the later stages (stage times, tags per frame).  Prints one JSON line.  The filter kernel's own time comes from a
separate `rocprofv3 --kernel-trace --stats -- python tools/bench_quad_sigma.py --filter-only` run (k_prefilter rows).

    python tools/bench_quad_sigma.py [--batch 256] [--steps 10] [--warmup 3] [--filter-only]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from chalkydri_amd import scenes
from chalkydri_amd.apriltags import AprilTags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--unique", type=int, default=32)
    ap.add_argument("--filter-only", action="store_true", help="only the front end (filter + threshold + segmentation), for a kernel trace")
    a = ap.parse_args()
    torch.cuda.init()
    w, h, n = 1280, 800, a.batch
    frames, gyro, layout, calib, r2c = scenes.bench_stream(2, n, w, h, 8, unique=a.unique, noise_amp=3)
    out = {"workload": f"{w}x{h}x{n}, 8 tags, noise+-3, detect+pose per step (bench.py's path)", "runs": []}
    for dec in (1, 2):
        task = AprilTags(w, h, layout, calib, r2c, cam_id=0, max_batch=n, quad_decimate=dec)
        det = task.detector
        det.upload(frames)
        for sigma in (0.0, 0.8, -0.8, 2.0):
            det.set_quad_sigma(sigma)
            fe = det.time_threshold_segment(n, iters=max(a.steps, 5))   # front end: filter (if on) + threshold + segmentation
            row = {"quad_decimate": dec, "sigma": sigma, "front_end_ms": round(fe, 4)}
            if not a.filter_only:
                for _ in range(a.warmup):
                    task.process_batch(None, gyro, n)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.steps):
                    recs, valid = task.process_batch(None, gyro, n)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / a.steps
                dets = det.detect_batch(None, n=n, cap=64)
                row.update({"ms_per_step": round(ms, 3), "frames_per_s": round(n / ms * 1e3, 1), "poses": int(np.sum(valid)),
                            "tags_per_frame": round(sum(len(d) for d in dets) / n, 3),
                            "stage_ms": {k: round(v, 3) for k, v in det.stage_ms().items()}})
            out["runs"].append(row)
        det.close()
    for r in out["runs"]:   # the filter's share of the front end: filtered minus unfiltered pass of the same decimation
        base = [b for b in out["runs"] if b["quad_decimate"] == r["quad_decimate"] and b["sigma"] == 0.0][0]
        r["front_end_delta_ms"] = round(r["front_end_ms"] - base["front_end_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
