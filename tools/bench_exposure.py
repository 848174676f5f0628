#!/usr/bin/env python3
"""Times ck_exposure_stats on a staged batch against what a caller would pay without it: the device-to-host copy of the same staged
frames (n * stride * h bytes into pinned memory, no host computation), and against ck_detect_uploaded of the same batch, all in
one process.   python tools/bench_exposure.py [N=256] [W=1280] [H=800] [ITERS=20]      One JSON line.
With CK_EXPOSURE_ONLY=1 only the metering runs (for a kernel trace of its own)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    n, w, h, iters = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 256), (2, 1280), (3, 800), (4, 20)))
    import torch
    from chalkydri_amd import scenes
    from chalkydri_amd.detector import AprilTagDetector
    frames = scenes.bench_stream(2, n, w, h, 6, unique=min(n, 16))[0]
    det = AprilTagDetector(w, h, max_batch=n)
    det.upload(frames)

    def timed(fn):
        for _ in range(3):
            fn()
        t = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        t.sort()
        return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1]}
    out = {"n": n, "w": w, "h": h, "iters": iters, "exposure_stats": timed(lambda: det.exposure_stats(n=n))}
    if not os.environ.get("CK_EXPOSURE_ONLY"):
        stride = (w + 15) // 16 * 16
        dev = torch.zeros(n * stride * h, dtype=torch.uint8, device="cuda")
        pinned = torch.empty(n * stride * h, dtype=torch.uint8).pin_memory()
        out["copy_bytes"] = n * stride * h
        out["d2h_copy"] = timed(lambda: pinned.copy_(dev, non_blocking=True))
        out["detect_uploaded"] = timed(lambda: det.detect_batch(None, n=n))
        out["stats_over_copy"] = out["exposure_stats"]["median_ms"] / out["d2h_copy"]["median_ms"]
        out["stats_over_detect"] = out["exposure_stats"]["median_ms"] / out["detect_uploaded"]["median_ms"]
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
