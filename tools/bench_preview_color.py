#!/usr/bin/env python3
"""Times the colour preview (ck_preview_jpeg_color: orient + convert + scale + FDCT + Huffman + stuffing on the device, from the
raw frames the last ck_upload_raw left there; only the files cross the bus) on 256 raw 1280x800 frames, YUYV and RGB3, to 640x480
quality 50, beside
  (a) ck_preview_jpeg (the grey file) on the same batch, and
  (b) the host's way: the raw frames copied out of device memory, converted and scaled in numpy, encoded by Pillow /
      libjpeg-turbo (mode YCbCr, 4:4:4) on 16 threads,
all in the same run.  The device files are byte-checked against (b) and against the restatement.  One JSON line per format;
`latency_n1_ms` is the median call of one frame.
Run it alone, and under `rocprofv3 --kernel-trace --stats -- python tools/bench_preview_color.py --iters 3` for the per-kernel split.
With --fourcc NV12 --planes (or NV21 / I420 / YV12) the frames are of that planar 4:2:0 format with their chroma planes (§4s);
--orientation turns the source; --no-host leaves the host's way out.
usage: python tools/bench_preview_color.py [--iters N] [--frames N] [--only FOURCC] [--fourcc FOURCC --planes] [--orientation NAME] [--no-host]"""
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
import torch  # noqa: E402  (one HIP runtime per process: torch's, as bench.py loads it)

import np_jpeg_enc_color as EC  # noqa: E402
import preview_color_ref as PC  # noqa: E402
import raw_planes_ref as P  # noqa: E402
import raw_format_ref as R  # noqa: E402
from chalkydri_amd import scenes  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402

W, H, PW, PH, Q = 1280, 800, 640, 480, 50


def camera_frame(scene, fourcc):
    """The raw frame a colour camera would deliver of the rendered scene: its luma with a little colour spread around it
    (raw_format_ref.grey_to_rgb), as RGB3 or, converted and with the chroma of every second pixel, as YUYV."""
    rgb = R.grey_to_rgb(scene, 3)
    if fourcc == "RGB3":
        return R.pack(rgb, fourcc)
    yc = EC.rgb_to_ycc(rgb)
    if fourcc in P.FOURCCS:                                 # ... or with the chroma of every second pixel of every second row
        return P.pack_planes(yc[..., 0], yc[0::2, 0::2, 1], yc[0::2, 0::2, 2], fourcc, W)
    buf = np.empty((H, 2 * W), np.uint8)
    buf[:, 0::2], buf[:, 1::4], buf[:, 3::4] = yc[..., 0], yc[:, 0::2, 1], yc[:, 0::2, 2]
    return buf


def median_ms(call, iters):
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def triples(f, fourcc, stride, o, pw, ph):
    """The restatement's preview triples of one raw frame."""
    if fourcc in P.FOURCCS:
        return P.preview(P.triples_vec(f, fourcc, W, H, stride, o), pw, ph)
    return PC.triples_vec(f, fourcc, W, H, stride, o, pw, ph)


def host_path(dev, n, fourcc, stride, iters, o, pw, ph, threads=16):
    """(median ms, files): D2H of the raw frames + conversion and nearest-neighbour scale in numpy + Pillow on `threads` threads."""
    from PIL import Image

    def enc(f):
        buf = io.BytesIO()
        Image.fromarray(triples(f, fourcc, stride, o, pw, ph), "YCbCr").save(buf, "JPEG", quality=Q, subsampling=0, optimize=False)
        return buf.getvalue()
    t = []
    with ThreadPoolExecutor(threads) as ex:
        for it in range(iters + 1):
            t0 = time.perf_counter()
            frames = dev.cpu().numpy().reshape(n, -1, stride)
            files = list(ex.map(enc, frames))
            if it:
                t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--only", default=None)
    ap.add_argument("--fourcc", default=None)
    ap.add_argument("--planes", action="store_true")
    ap.add_argument("--orientation", default="none")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if args.planes != (args.fourcc in P.FOURCCS):
        raise SystemExit("--planes goes with --fourcc NV12 / NV21 / I420 / YV12, and they with it")
    o = args.orientation
    ow, oh = (H, W) if o in ("clockwise", "counterclockwise") else (W, H)
    pw, ph = (PH, PW) if (ow, oh) != (W, H) else (PW, PH)
    n = args.frames
    uniq = scenes.bench_stream(1, 4, W, H, 12, unique=4)[0]
    det = AprilTagDetector(ow, oh, max_batch=n)
    kw = dict(width=pw, height=ph, quality=Q)
    for fourcc in (args.fourcc,) if args.fourcc else ("YUYV", "RGB3"):
        if args.only and fourcc != args.only:
            continue
        src = [camera_frame(f, fourcc) for f in uniq]
        stride = src[0].shape[1]
        raw = [src[i % len(src)] for i in range(n)]
        det.upload_raw(raw, fourcc, o, planes=args.planes)
        for _ in range(3):
            files = det.preview_jpeg_color(n=n, **kw)
            det.preview_jpeg_color(n=1, **kw)
            det.preview_jpeg(n=n, **kw)
        m, mn = median_ms(lambda: det.preview_jpeg_color(n=n, **kw), args.iters)
        lat, _ = median_ms(lambda: det.preview_jpeg_color(n=1, **kw), args.iters)
        grey, _ = median_ms(lambda: det.preview_jpeg(n=n, **kw), args.iters)
        grey1, _ = median_ms(lambda: det.preview_jpeg(n=1, **kw), args.iters)
        files = det.preview_jpeg_color(n=n, **kw)
        exact = all(files[i] == EC.encode_ycc(triples(raw[i], fourcc, stride, o, pw, ph), Q, 0) for i in range(len(src)))
        if args.no_host:
            print(json.dumps({"format": fourcc, "planes": args.planes, "orientation": o, "frames": n, "preview": [pw, ph], "quality": Q,
                              "files_MB": round(sum(len(b) for b in files) / 1e6, 2), "preview_jpeg_color_ms": round(m, 3),
                              "preview_jpeg_color_min_ms": round(mn, 3), "frames_per_s": round(n / m * 1e3, 1), "latency_n1_ms": round(lat, 3),
                              "grey_preview_jpeg_ms": round(grey, 3), "color_over_grey": round(m / grey, 2), "byte_exact": exact}), flush=True)
            continue
        dev = torch.from_numpy(np.stack(raw)).cuda()          # the raw frames as a caller holds them on the device
        torch.cuda.synchronize()
        host = host_path(dev, n, fourcc, stride, max(3, args.iters // 4), o, pw, ph)
        print(json.dumps({"format": fourcc, "planes": args.planes, "orientation": o, "frames": n, "preview": [pw, ph], "quality": Q, "files_MB": round(sum(len(b) for b in files) / 1e6, 2),
                          "preview_jpeg_color_ms": round(m, 3), "preview_jpeg_color_min_ms": round(mn, 3), "frames_per_s": round(n / m * 1e3, 1),
                          "latency_n1_ms": round(lat, 3), "grey_preview_jpeg_ms": round(grey, 3), "grey_latency_n1_ms": round(grey1, 3),
                          "color_over_grey": round(m / grey, 2), "host_d2h_numpy_pillow_16_threads_ms": round(host[0], 3),
                          "speedup_vs_host_path": round(host[0] / m, 2), "byte_exact": exact, "host_files_equal": host[1] == files}), flush=True)
        del dev
    det.close()


if __name__ == "__main__":
    main()
