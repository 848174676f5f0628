#!/usr/bin/env python3
"""What the JPEG ingest ring hides: steady-state milliseconds per step of 256 frames of 1280x800, q85 4:2:0 (the bench
workload's scenes, scenes.bench_stream) for
  (a) upload_then_process   ck_upload_jpeg, then ck_process_uploaded: parse, copy, decode and detect + pose one after the other;
  (b) ring                  a two-slot JPEG ring: ck_ingest_write_jpeg x n + ck_ingest_submit of slot k+1, then
                            ck_process_ingested of slot k, so that slot k+1's copy and decode run on the ring's stream beside it.
Host wall clock over `--steps` steps after `--warmup`, (a) and (b) alternating, `--runs` runs each; the host time of the n
ck_ingest_write_jpeg calls (parse + copy into pinned memory) and of ck_ingest_submit is reported beside them.  The C entry points
are called on prebuilt arguments, so that neither side pays for Python's copies.  One JSON line.
  --trace   instead: three oriented uploads per orientation (the 1280x800 streams into a 1280x800 handle for none / rotate-180 and
            into an 800x1280 handle for the quarter turns), for `rocprofv3 --kernel-trace --stats -- python tools/bench_jpeg_ring.py
            --trace`: the four k_jpeg_idct instantiations in one trace.
usage: python tools/bench_jpeg_ring.py [--frames N] [--steps N] [--warmup N] [--runs N] [--orientation NAME] [--trace]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one HIP runtime per process: torch's, as bench.py loads it)

import np_jpeg as J  # noqa: E402
import raw_format_ref as R  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd import scenes  # noqa: E402
from chalkydri_amd.apriltags import AprilTags  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector, IngestRing, _jpeg_frames, orientation_code  # noqa: E402


def trace(streams, w, h, n):
    for o in R.ORIENTATIONS:
        W, H = (h, w) if o in ("clockwise", "counterclockwise") else (w, h)
        det = AprilTagDetector(W, H, max_batch=n)
        for _ in range(3):
            det.upload_jpeg(streams, o)
        det.close()
    print(json.dumps({"trace": "k_jpeg_idct", "frames": n, "uploads_per_orientation": 3}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--orientation", default="none")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    w, h, n = 1280, 800, args.frames
    o = args.orientation
    frames, gyro, layout, calib, r2c = scenes.bench_stream(1, n, w, h, 12, unique=4)
    uniq = [J.encode(R.source_of(frames[i], o), sampling="420", quality=85) for i in range(4)]
    streams = [uniq[i % 4] for i in range(n)]
    if args.trace:
        return trace(streams, w, h, n)   # (--orientation stays "none": the handles' geometry does the turning)
    task = AprilTags(w, h, layout, calib, r2c, cam_id=1, max_batch=n)
    det, L = task.detector, task.detector._L
    oc = orientation_code(o)
    arr, keep = _jpeg_frames(streams)
    ring = IngestRing(det, 2, fourcc="MJPG", orientation=o, max_frame_bytes=max(len(b) for b in streams) + 4096)
    g = np.ascontiguousarray(gyro, np.float64)
    has = np.ones(n, np.uint8)
    out = (A.VisionMeasurement * n)()
    valid = (C.c_int32 * n)()
    st = (C.c_uint32 * n)()
    t_write, t_submit = [], []

    def step_a():
        assert L.ck_upload_jpeg_oriented(det._h, arr, n, oc, st) == 0
        assert L.ck_process_uploaded(det._h, n, C.byref(task._pp), g.ctypes.data, has.ctypes.data, out, valid) == 0

    def fill(slot):
        t0 = time.perf_counter()
        for i in range(n):
            assert L.ck_ingest_write_jpeg(ring._g, slot, i, arr[i].data, arr[i].size) == 0
        t1 = time.perf_counter()
        assert L.ck_ingest_submit(ring._g, slot, n) == 0
        t_write.append((t1 - t0) * 1e3)
        t_submit.append((time.perf_counter() - t1) * 1e3)

    def step_b(k):
        fill((k + 1) % 2)
        assert L.ck_process_ingested(ring._g, k % 2, n, C.byref(task._pp), g.ctypes.data, has.ctypes.data, out, valid) == 0

    step_a()
    rec_a = bytes(out)
    fill(0)
    step_b(0)
    same = bytes(out) == rec_a
    res = {"a": [], "b": []}
    k = 1
    for run in range(args.runs):
        for _ in range(args.warmup):
            step_a()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step_a()
        res["a"].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for _ in range(args.warmup):
            step_b(k); k += 1
        del t_write[:], t_submit[:]
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step_b(k); k += 1
        res["b"].append((time.perf_counter() - t0) * 1e3 / args.steps)
    same = same and bytes(out) == rec_a
    L.ck_process_ingested(ring._g, k % 2, n, C.byref(task._pp), g.ctypes.data, has.ctypes.data, out, valid)   # (drain the slot in flight)
    ring.close()
    det.close()
    a, b = res["a"], res["b"]
    print(json.dumps({"bench": "jpeg_ring", "frames": n, "width": w, "height": h, "orientation": o, "steps": args.steps,
                      "compressed_MB": round(sum(len(s) for s in streams) / 1e6, 2),
                      "upload_then_process_ms": [round(v, 3) for v in a], "ring_ms": [round(v, 3) for v in b],
                      "upload_then_process_mean_ms": round(float(np.mean(a)), 3), "ring_mean_ms": round(float(np.mean(b)), 3),
                      "upload_then_process_spread_ms": round(max(a) - min(a), 3),
                      "ring_saves_ms": round(float(np.mean(a) - np.mean(b)), 3),
                      "write_jpeg_host_ms_per_step": round(float(np.median(t_write)), 3),
                      "submit_host_ms_per_step": round(float(np.median(t_submit)), 3), "records_equal": same}), flush=True)


if __name__ == "__main__":
    main()
