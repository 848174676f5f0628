#!/usr/bin/env python3
"""Times the per-tag pose kernel (k_tagpose.hip) through ck_estimate_tag_poses on device-resident detections and records, for
two batches: 256 frames x 6 tags (the bench.py workload) and 512 x 30 (BASELINE config 3).  The detections are exact
projections of random poses (the kernel's work does not depend on where the corners came from).  Prints one JSON line per
batch: median / min milliseconds per call, which include a 96-byte-per-detection device copy in and the records' copy out.
Run it alone, and under `rocprofv3 --kernel-trace --stats -- python tools/bench_tag_pose.py` for the kernel time itself.
usage: python tools/bench_tag_pose.py [--iters N]"""
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
import torch  # noqa: E402

import tag_pose_util as U  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector, tag_pose_params  # noqa: E402


def detections(n, cam, rng):
    arr = (A.Detection * n)()
    for k in range(n):
        R, t = U.random_pose(rng, 0.5, 8.0)
        c = U.project(R, t, 0.1651 / 2, cam)
        arr[k].id = k % 587
        for i in range(4):
            arr[k].p[i][0], arr[k].p[i][1] = c[i]
    return arr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    torch.cuda.init()
    cam = (1000.0, 1000.0, 640.0, 400.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    pp = tag_pose_params(*cam[:4])
    rng = np.random.default_rng(1)
    det = AprilTagDetector(320, 240, max_batch=512)
    for frames, tags in ((256, 6), (512, 30)):
        n = frames * tags
        host = detections(n, cam, rng)
        d_dets = torch.from_numpy(np.frombuffer(bytes(host), np.uint8).copy()).cuda()
        d_out = torch.zeros(n * C.sizeof(A.TagPose), dtype=torch.uint8, device="cuda")
        call = lambda: det._L.ck_estimate_tag_poses(det._h, C.byref(pp), C.c_void_p(d_dets.data_ptr()), n, C.c_void_p(d_out.data_ptr()))
        assert call() == 0
        ms = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            assert call() == 0
            ms.append((time.perf_counter() - t0) * 1e3)
        rec = (A.TagPose * n).from_buffer_copy(d_out.cpu().numpy().tobytes())
        valid = sum(r.valid for r in rec)
        print(json.dumps({"batch": f"{frames}x{tags}", "detections": n, "valid": valid, "median_ms": round(float(np.median(ms)), 4),
                          "min_ms": round(float(np.min(ms)), 4), "iters": args.iters}), flush=True)


if __name__ == "__main__":
    main()
