#!/usr/bin/env python3
"""Times ck_cat_tri_otsu_batch on RGB frames resident on the device — one frame and a batch — against a device-to-device copy of
the bytes its three kernels read and write (3 + 3 + 1 per pixel; the copy reads and writes each of them, so it moves twice that
traffic), and, on one frame in host memory, against ck_cat_calc_otsu, the function it stands beside, all in one process.
    python tools/bench_cat_threshold.py [N=64] [W=1280] [H=800] [ITERS=20] [REPS=50]      One JSON line.
A sample is the host clock around REPS back-to-back calls that end in a device synchronise, divided by REPS (one call is tens of
microseconds: a window of one would time the clock); the figures are the median, minimum and maximum of ITERS samples after warm-up.
With CK_TRI_ONLY=1 only the batched call runs (for a kernel trace of its own)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    n, w, h, iters, reps = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 64), (2, 1280), (3, 800), (4, 20), (5, 50)))
    import numpy as np
    import torch
    from chalkydri_amd import scenes
    from chalkydri_amd.cat import CatDetector
    grey = scenes.bench_stream(2, n, w, h, 6, unique=min(n, 16))[0]
    rng = np.random.default_rng(1)
    rgb = np.clip(np.repeat(grey[..., None], 3, axis=3).astype(np.int16) + rng.integers(-3, 4, (1, h, w, 3)), 0, 255).astype(np.uint8)
    det = CatDetector(w, h)
    dev = torch.from_numpy(rgb).cuda()

    def timed(fn):
        for _ in range(3):
            fn()
        t = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3 / reps)
        t.sort()
        return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1]}
    out = {"n": n, "w": w, "h": h, "iters": iters, "reps": reps, "tri_otsu_batch_device": timed(lambda: det.tri_otsu_batch(dev))}
    if not os.environ.get("CK_TRI_ONLY"):
        out["tri_otsu_one_device"] = timed(lambda: det.tri_otsu_batch(dev[:1]))
        for name, k in (("d2d_copy_batch", n), ("d2d_copy_one", 1)):
            a = torch.zeros(7 * k * w * h, dtype=torch.uint8, device="cuda")
            b = torch.empty_like(a)
            out[name] = dict(timed(lambda: (b.copy_(a), torch.cuda.synchronize())), bytes=7 * k * w * h)   # (complete on return, as the library's call)
        out["tri_otsu_one_host"] = timed(lambda: det.tri_otsu(rgb[0]))
        out["calc_otsu_one_host"] = timed(lambda: det.calc_otsu(rgb[0]))
        out["batch_over_copy"] = out["tri_otsu_batch_device"]["median_ms"] / out["d2d_copy_batch"]["median_ms"]
        out["one_over_copy"] = out["tri_otsu_one_device"]["median_ms"] / out["d2d_copy_one"]["median_ms"]
        out["calc_otsu_over_tri_otsu_host"] = out["calc_otsu_one_host"]["median_ms"] / out["tri_otsu_one_host"]["median_ms"]
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
