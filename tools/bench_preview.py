#!/usr/bin/env python3
"""Times the device JPEG preview (ck_preview_jpeg: scale + overlay + FDCT + Huffman + stuffing on the device, only the files
cross the bus) on 256 staged 1280x800 frames of bench-style scenes (scenes.bench_stream, a few distinct frames repeated), beside
the alternative a caller has without it — the staged frames copied to the host (ck_quad_image_batch on the staged frames), scaled
by nearest neighbour and encoded by Pillow / libjpeg-turbo on 16 threads — and beside ck_detect_uploaded on the same batch, all
in the same run.  One JSON line per workload:
  stream_640x480_q50          the reference's driver-station stream
  stream_640x480_q50_overlay  the same with the detections outlined
  stream_640x480_q50_rst1     the same with a restart interval of one block row
  full_1280x800_q85           no scaling, quality 85
Every line also has `latency_n1_ms`: the median ck_preview_jpeg of one frame.
Run it alone, and under `rocprofv3 --kernel-trace --stats -- python tools/bench_preview.py --iters 3` for the per-kernel split.
usage: python tools/bench_preview.py [--iters N] [--frames N] [--only NAME]"""
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

import np_jpeg_enc as E  # noqa: E402
from chalkydri_amd import scenes  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402

W, H = 1280, 800
WORKLOADS = [("stream_640x480_q50", dict(width=640, height=480, quality=50)),
             ("stream_640x480_q50_overlay", dict(width=640, height=480, quality=50, overlay=True)),
             ("stream_640x480_q50_rst1", dict(width=640, height=480, quality=50, restart_rows=1)),
             ("full_1280x800_q85", dict(width=0, height=0, quality=85))]


def host_path_ms(det, n, kw, iters, threads=16):
    """D2H of the staged frames + nearest-neighbour scale + Pillow encode on `threads` threads; None without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return None
    pw, ph, _ = E.layout(kw["width"], kw["height"], W, H)
    sy = ((2 * np.arange(ph) + 1) * H) // (2 * ph)
    sx = ((2 * np.arange(pw) + 1) * W) // (2 * pw)
    extra = {"restart_marker_rows": kw["restart_rows"]} if kw.get("restart_rows") else {}

    def enc(f):
        buf = io.BytesIO()
        P = f if (pw, ph) == (W, H) else f[sy][:, sx]
        Image.fromarray(P).save(buf, "JPEG", quality=kw["quality"], optimize=False, **extra)
        return buf.getvalue()
    t = []
    with ThreadPoolExecutor(threads) as ex:
        for it in range(iters + 1):
            t0 = time.perf_counter()
            frames = det.quad_image(None, n=n)          # quad_decimate 1, no filter: the staged frames themselves
            files = list(ex.map(enc, frames))
            if it:
                t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    n = args.frames
    uniq = scenes.bench_stream(1, 4, W, H, 12, unique=4)[0]
    frames = np.stack([uniq[i % len(uniq)] for i in range(n)])
    det = AprilTagDetector(W, H, max_batch=n)
    det.upload(frames)
    dets = det.detect_batch(None, n=n)
    dt = []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        det.detect_batch(None, n=n)
        dt.append((time.perf_counter() - t0) * 1e3)
    detect_ms = float(np.median(dt))
    for name, kw in WORKLOADS:
        if args.only and name != args.only:
            continue
        for _ in range(3):
            files = det.preview_jpeg(n=n, **kw)
            det.preview_jpeg(n=1, **kw)
        ms, lat = [], []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            files = det.preview_jpeg(n=n, **kw)          # returns after the stream is synchronised and the files are on the host
            ms.append((time.perf_counter() - t0) * 1e3)
        for _ in range(args.iters):
            t0 = time.perf_counter()
            det.preview_jpeg(n=1, **kw)
            lat.append((time.perf_counter() - t0) * 1e3)
        pw, ph, _ = E.layout(kw["width"], kw["height"], W, H)
        exact = all(files[i] == E.encode_grey(E.preview(frames[i], pw, ph, [d.corners() for d in dets[i]] if kw.get("overlay") else None),
                                              kw["quality"], kw.get("restart_rows", 0)) for i in range(min(n, len(uniq))))
        host = None if kw.get("overlay") else host_path_ms(det, n, kw, max(3, args.iters // 4))   # (Pillow draws no outlines)
        m = float(np.median(ms))
        line = {"workload": name, "frames": n, "preview": [pw, ph], "files_MB": round(sum(len(b) for b in files) / 1e6, 2),
                "preview_jpeg_ms": round(m, 3), "preview_jpeg_min_ms": round(float(np.min(ms)), 3),
                "frames_per_s": round(n / m * 1e3, 1), "latency_n1_ms": round(float(np.median(lat)), 3),
                "detect_uploaded_ms": round(detect_ms, 3), "share_of_detect": round(m / detect_ms, 3),
                "host_d2h_scale_pillow_16_threads_ms": None, "speedup_vs_host_path": None, "byte_exact": exact}
        if host is not None:
            line["host_d2h_scale_pillow_16_threads_ms"] = round(host[0], 3)
            line["speedup_vs_host_path"] = round(host[0] / m, 2)
            line["host_files_equal"] = host[1][:len(uniq)] == files[:len(uniq)]
        print(json.dumps(line), flush=True)
    det.close()


if __name__ == "__main__":
    main()
