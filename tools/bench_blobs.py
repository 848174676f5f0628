#!/usr/bin/env python3
"""Coloured game pieces: the numbers of DESIGN.md §4r.

    python tools/bench_blobs.py [N] [--fourcc YUYV|NV12|NV21|I420|YV12 --planes] [--orientation NAME] [--no-host]
        N (256) frames of 1280 x 800 resident on the device (YUYV, or a planar 4:2:0 format with its chroma planes, §4s; turned by
        the orientation), with one class and with four:
        kernel_ms   ck_blob_time: the kernels of one ck_detect_blobs_device call between two events on the handle's stream
        copy_ms     a device-to-device copy that moves the bytes the kernels must touch: 2 B / px of raw frame read, every class's
                    plane written once and read by the five word passes (6 x 1 / 8 B / px per class); the label traffic is
                    per run, not per pixel, and is left out: the bound is a lower one
        host_ms     the path the feature replaces: the raw frames copied out, then ck_blobs_host on 16 threads (its RGB input is
                    taken from ck_blob_rgb and not counted, which flatters the host)
One JSON line."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1280, 800


def scene(rng, fourcc="YUYV"):
    """One frame: a grey, slightly noisy field with a dozen saturated pieces of four colours; YUYV, or (the chroma of every second
    row) one of the planar 4:2:0 formats with its planes."""
    y = np.clip(rng.normal(110, 20, (H, W)), 0, 255).astype(np.uint8)
    u = np.clip(rng.normal(128, 3, (H, W // 2)), 0, 255).astype(np.uint8)
    v = np.clip(rng.normal(128, 3, (H, W // 2)), 0, 255).astype(np.uint8)
    for k in range(12):
        x0, y0 = int(rng.integers(0, W - 160)) & ~1, int(rng.integers(0, H - 120))
        w, h = int(rng.integers(20, 160)) & ~1, int(rng.integers(20, 120))
        yy, uu, vv = ((150, 60, 200), (160, 60, 60), (100, 220, 110), (200, 30, 150))[k % 4]   # orange, green, blue, yellow
        y[y0:y0 + h, x0:x0 + w] = yy
        u[y0:y0 + h, x0 // 2:(x0 + w) // 2] = uu
        v[y0:y0 + h, x0 // 2:(x0 + w) // 2] = vv
    if fourcc != "YUYV":
        import raw_planes_ref as P
        return P.pack_planes(y, u[0::2], v[0::2], fourcc, W)
    out = np.empty((H, W * 2), np.uint8)
    out[:, 0::2] = y
    out[:, 1::4] = u
    out[:, 3::4] = v
    return out


def main(n, fourcc="YUYV", planes=False, orientation="none", host=True):
    import torch
    from chalkydri_amd import blobs as B
    from chalkydri_amd.detector import AprilTagDetector
    if (fourcc != "YUYV") != planes:
        raise SystemExit("the planar formats go with --planes, YUYV without")
    rng = np.random.default_rng(0)
    base = np.stack([scene(rng, fourcc) for _ in range(8)])
    dev = torch.from_numpy(base).cuda().repeat((n + 7) // 8, 1, 1)[:n].contiguous()
    torch.cuda.synchronize()
    ow, oh = (H, W) if orientation in ("clockwise", "counterclockwise") else (W, H)
    det = AprilTagDetector(ow, oh, max_batch=n)
    stride, rows = base.shape[2], base.shape[1]
    src = (dev.data_ptr(), n, stride, stride * rows, fourcc, orientation)
    bpp = stride * rows / (W * H)                      # bytes of raw frame per pixel: 2 for YUYV, 1.5 for the 4:2:0 formats
    palette = [B.ColorClass(h_min=5, h_max=25, min_area=64), B.ColorClass(h_min=45, h_max=75, min_area=64),
               B.ColorClass(h_min=105, h_max=130, min_area=64), B.ColorClass(h_min=26, h_max=40, min_area=64)]
    out = {"frames": n, "size": [W, H], "fourcc": fourcc, "planes": planes, "orientation": orientation}
    for nc in (1, 4):
        pp = B.blob_params(palette[:nc], erode=1, dilate=1)
        kernel_ms = det.blob_time(pp, *src, reps=5, planes=planes)
        rec, counts, status = det.detect_blobs_device(pp, *src, planes=planes)
        moved = int(n * W * H * (bpp + nc * 6 / 8))
        a = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        b = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        b.copy_(a)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(5):
            b.copy_(a)
        ev[1].record()
        torch.cuda.synchronize()
        copy_ms = ev[0].elapsed_time(ev[1]) / 5
        del a, b
        if not host:
            out[f"classes_{nc}"] = {"kernel_ms": round(kernel_ms, 3), "bytes_moved": moved, "copy_ms": round(copy_ms, 3),
                                    "targets": int(counts.sum()), "flagged": int((status != 0).sum())}
            continue
        # the replaced path
        nh = min(n, 64)                                   # (the host part on a quarter of the frames, scaled: it is linear in n)
        rgb = det.blob_rgb(n=nh, device=src + (planes,))
        t0 = time.perf_counter()
        host_raw = dev.cpu()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            res = list(ex.map(lambda i: B.blobs_host(pp, rgb[i:i + 1]), range(nh)))
        t_host = (time.perf_counter() - t0) * n / nh
        assert all(np.array_equal(res[i][1][0], counts[i]) for i in range(nh)) and host_raw.shape[0] == n
        out[f"classes_{nc}"] = {"kernel_ms": round(kernel_ms, 3), "bytes_moved": moved, "copy_ms": round(copy_ms, 3),
                                "copy_out_ms": round(t_copy * 1e3, 1), "host16_ms": round(t_host * 1e3, 1),
                                "host_ms": round((t_copy + t_host) * 1e3, 1), "targets": int(counts.sum()), "flagged": int((status != 0).sum())}
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("frames", nargs="?", type=int, default=256)
    ap.add_argument("--fourcc", default="YUYV")
    ap.add_argument("--planes", action="store_true")
    ap.add_argument("--orientation", default="none")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    main(a.frames, a.fourcc, a.planes, a.orientation, not a.no_host)
