#!/usr/bin/env python3
"""Coloured game pieces: the numbers of DESIGN.md §4r.

    python tools/bench_blobs.py [N]      N (256) YUYV frames of 1280 x 800 resident on the device, with one class and with four:
        kernel_ms   ck_blob_time: the kernels of one ck_detect_blobs_device call between two events on the handle's stream
        copy_ms     a device-to-device copy that moves the bytes the kernels must touch: 2 B / px of raw frame read, every class's
                    plane written once and read by the five word passes (6 x 1 / 8 B / px per class); the label traffic is
                    per run, not per pixel, and is left out: the bound is a lower one
        host_ms     the path the feature replaces: the raw frames copied out, then ck_blobs_host on 16 threads (its RGB input is
                    taken from ck_blob_rgb and not counted, which flatters the host)
One JSON line."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1280, 800


def scene(rng):
    """One YUYV frame: a grey, slightly noisy field with a dozen saturated pieces of four colours."""
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
    out = np.empty((H, W * 2), np.uint8)
    out[:, 0::2] = y
    out[:, 1::4] = u
    out[:, 3::4] = v
    return out


def main(n):
    import torch
    from chalkydri_amd import blobs as B
    from chalkydri_amd.detector import AprilTagDetector
    rng = np.random.default_rng(0)
    base = np.stack([scene(rng) for _ in range(8)])
    dev = torch.from_numpy(base).cuda().repeat((n + 7) // 8, 1, 1)[:n].contiguous()
    torch.cuda.synchronize()
    det = AprilTagDetector(W, H, max_batch=n)
    src = (dev.data_ptr(), n, 2 * W, 2 * W * H, "YUYV", "none")
    palette = [B.ColorClass(h_min=5, h_max=25, min_area=64), B.ColorClass(h_min=45, h_max=75, min_area=64),
               B.ColorClass(h_min=105, h_max=130, min_area=64), B.ColorClass(h_min=26, h_max=40, min_area=64)]
    out = {"frames": n, "size": [W, H], "fourcc": "YUYV"}
    for nc in (1, 4):
        pp = B.blob_params(palette[:nc], erode=1, dilate=1)
        kernel_ms = det.blob_time(pp, *src, reps=5)
        rec, counts, status = det.detect_blobs_device(pp, *src)
        moved = int(n * W * H * (2 + nc * 6 / 8))
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
        # the replaced path
        nh = min(n, 64)                                   # (the host part on a quarter of the frames, scaled: it is linear in n)
        rgb = det.blob_rgb(n=nh, device=src)
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
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 256)
