#!/usr/bin/env python3
"""Measurements of the colour form of the JPEG decode on §4c's batches: 256 x 1280x800 bench-style scenes with
chroma, q85 4:2:0 and q95 4:4:4.  One JSON line per measurement:
  decode   ck_upload_jpeg_color against ck_upload_jpeg_oriented, alternating in the same run: the price of the chroma
  preview  ck_upload_jpeg_color + ck_preview_jpeg_color (640 x 480, quality 50) against the host path it replaces on 16 threads:
           Pillow decode to YCbCr, numpy nearest-neighbour scale, Pillow encode
  luma     (--luma-only) ck_upload_jpeg alone on the q85 4:2:0 batch.  With --tree PATH the package and the library of another
           checkout (the parent commit, built) are loaded instead of this one's: run the two alternately and compare the spreads.
usage: python tools/bench_jpeg_color.py [--iters N] [--frames N] [--luma-only] [--tree PATH]"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--luma-only", action="store_true")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one HIP runtime per process: torch's, as bench.py loads it)

import np_jpeg as J  # noqa: E402
from chalkydri_amd import scenes  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402

W, H = 1280, 800
WORKLOADS = [("q85_420", dict(sampling="420", quality=85)), ("q95_444", dict(sampling="444", quality=95))]


def batch(kw, nf):
    frames = scenes.bench_stream(1, 4, W, H, 12, unique=4)[0]
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:H, 0:W]
    uniq = []
    for f in frames:   # chroma: two smooth fields with a little noise, as a camera's is
        ch = [np.clip(128 + 60 * np.sin(xx / rng.uniform(40, 90) + yy / rng.uniform(50, 120)) + rng.normal(0, 4, (H, W)), 0, 255).astype(np.uint8)
              for _ in range(2)]
        uniq.append(J.encode(f, chroma=tuple(ch), **kw))
    return [uniq[i % len(uniq)] for i in range(nf)]


def stats(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(np.min(t)), 3), "max_ms": round(float(np.max(t)), 3)}


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def host_preview_ms(streams, threads=16):
    from PIL import Image
    sy = ((2 * np.arange(480) + 1) * H) // (2 * 480)
    sx = ((2 * np.arange(640) + 1) * W) // (2 * 640)

    def one(b):
        im = Image.open(io.BytesIO(b))
        im.draft("YCbCr", im.size)
        P = np.ascontiguousarray(np.asarray(im)[sy][:, sx])
        out = io.BytesIO()
        Image.fromarray(P, "YCbCr").save(out, "JPEG", quality=50, subsampling=0)
        return out.tell()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, streams[:threads]))
        return [timed(lambda: list(ex.map(one, streams))) for _ in range(3)]


def main():
    nf = args.frames
    det = AprilTagDetector(W, H, max_batch=nf)
    for name, kw in WORKLOADS:
        streams = batch(kw, nf)
        if args.luma_only:
            if name != "q85_420":
                continue
            for _ in range(2):
                det.upload_jpeg(streams)
            t = [timed(lambda: det.upload_jpeg(streams)) for _ in range(args.iters)]
            print(json.dumps({"measure": "luma", "tree": ROOT, "workload": name, "frames": nf, **stats(t)}), flush=True)
            continue
        for _ in range(2):
            det.upload_jpeg(streams)
            det.upload_jpeg(streams, color=True)
            det.preview_jpeg_color(n=nf)
        luma, color, whole = [], [], []
        for _ in range(args.iters):
            luma.append(timed(lambda: det.upload_jpeg(streams)))
            color.append(timed(lambda: det.upload_jpeg(streams, color=True)))
        print(json.dumps({"measure": "decode", "workload": name, "frames": nf, "luma": stats(luma), "color": stats(color),
                          "color_over_luma": round(float(np.median(color) / np.median(luma)), 3)}), flush=True)
        for _ in range(args.iters):
            whole.append(timed(lambda: (det.upload_jpeg(streams, color=True), det.preview_jpeg_color(n=nf))))
        host = host_preview_ms(streams)
        print(json.dumps({"measure": "preview", "workload": name, "frames": nf, "device": stats(whole), "host_16_threads": stats(host),
                          "speedup": round(float(np.median(host) / np.median(whole)), 2)}), flush=True)
    det.close()


if __name__ == "__main__":
    main()
