#!/usr/bin/env python3
"""Times the device JPEG decode (ck_upload_jpeg: host parse + one copy + k_jpeg_frame + k_jpeg_idct) on 256-frame batches of
bench-style scenes (scenes.bench_stream, a few distinct frames repeated), beside ck_detect_uploaded on the same batch and, when
Pillow is importable, Pillow's luma decode of the same frames on 16 threads, all in the same run.  One JSON line per workload:
  q85_420            256 x 1280x800, q85 4:2:0, no DRI
  q85_420_dri_row    the same with a restart interval of one MCU row
  q95_444            256 x 1280x800, q95 4:4:4
  q85_420_1600       256 x 1600x1304, q85 4:2:0
  worst_noise_junk   16 x 1280x800, q100 4:4:4 of uniform noise (the densest scan a baseline encoder writes) with 4 MB of
                     junk between the last MCU and EOI (no marker in it: the device reads it as scan)
Every line also has `latency_n1_ms`: the median ck_upload_jpeg of one frame (the per-sample use).
Run it alone, and under `rocprofv3 --kernel-trace --stats -- python tools/bench_jpeg.py` for the per-kernel split.
usage: python tools/bench_jpeg.py [--iters N] [--frames N] [--only NAME]"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one HIP runtime per process: torch's, as bench.py loads it)

import np_jpeg as J  # noqa: E402
from chalkydri_amd import scenes  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402

WORKLOADS = [("q85_420", 1280, 800, dict(sampling="420", quality=85)),
             ("q85_420_dri_row", 1280, 800, dict(sampling="420", quality=85, restart_interval=1, restart_rows=True)),
             ("q95_444", 1280, 800, dict(sampling="444", quality=95)),
             ("q85_420_1600", 1600, 1304, dict(sampling="420", quality=85)),
             ("worst_noise_junk", 1280, 800, dict(sampling="444", quality=100))]


def pillow_ms(streams, threads=16):
    try:
        from PIL import Image
    except ImportError:
        return None

    def dec(b):
        im = Image.open(io.BytesIO(b))
        im.draft("L", im.size)
        im.load()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(dec, streams[:threads]))
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            list(ex.map(dec, streams))
            t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    for name, w, h, kw in WORKLOADS:
        if args.only and name != args.only:
            continue
        nf = args.frames
        if name == "worst_noise_junk":
            nf = min(nf, 16)
            b = J.encode((np.random.default_rng(5).random((h, w)) * 256).astype(np.uint8), **kw)
            junk = np.random.default_rng(6).integers(0, 255, 4 << 20, dtype=np.uint8).tobytes()   # no 0xFF: never a marker
            uniq = [b[:-2] + junk + b[-2:]]
        else:
            frames = scenes.bench_stream(1, 4, w, h, 12, unique=4)[0]
            uniq = [J.encode(f, **kw) for f in frames]
        streams = [uniq[i % len(uniq)] for i in range(nf)]
        mb = sum(len(b) for b in streams) / 1e6
        n = nf
        det = AprilTagDetector(w, h, max_batch=n)
        for _ in range(2):
            det.upload_jpeg(streams)
            det.detect_batch(None, n=n)
        lat = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            det.upload_jpeg(streams[:1])
            lat.append((time.perf_counter() - t0) * 1e3)
        up, dt = [], []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            det.upload_jpeg(streams)            # returns after the stream is synchronised
            t1 = time.perf_counter()
            det.detect_batch(None, n=n)
            t2 = time.perf_counter()
            up.append((t1 - t0) * 1e3)
            dt.append((t2 - t1) * 1e3)
        got = det.decode_jpeg(streams[:len(uniq)])
        exact = all(np.array_equal(got[i], J.decode_luma(uniq[i])[0]) for i in range(len(uniq)))
        det.close()
        ms = float(np.median(up))
        pil = pillow_ms(streams)
        print(json.dumps({"workload": name, "frames": n, "width": w, "height": h, "compressed_MB": round(mb, 2),
                          "upload_jpeg_ms": round(ms, 3), "upload_jpeg_min_ms": round(float(np.min(up)), 3),
                          "frames_per_s": round(n / ms * 1e3, 1), "compressed_MB_per_s": round(mb / ms * 1e3, 1),
                          "detect_uploaded_ms": round(float(np.median(dt)), 3), "latency_n1_ms": round(float(np.median(lat)), 3),
                          "pillow_16_threads_ms": None if pil is None else round(pil, 3),
                          "speedup_vs_pillow": None if pil is None else round(pil / ms, 2), "bit_exact": exact}), flush=True)


if __name__ == "__main__":
    main()
