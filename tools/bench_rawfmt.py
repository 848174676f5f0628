#!/usr/bin/env python3
"""Raw formats -> oriented luma: the numbers of DESIGN.md §4d.

    python tools/bench_rawfmt.py kernels [N]     every family x orientation once from device memory, N frames of 1280 x 800 (256),
                                                 and device-to-device copies of the same byte counts: run it under
                                                 `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python tools/bench_rawfmt.py kernels`
                                                 and read the kernel / copy times from the trace, not from this script's wall clock
    python tools/bench_rawfmt.py calls [N]       whole calls from pageable host memory, YUYV and RGB3: ck_upload_raw beside "convert on
                                                 the host on 16 threads, then ck_upload_frames"; wall time and host CPU seconds
One JSON line per mode."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raw_format_ref as R  # noqa: E402

W, H = 1280, 800


def kernels(n):
    import torch
    from chalkydri_amd.detector import AprilTagDetector
    dets = {(W, H): AprilTagDetector(W, H, max_batch=n), (H, W): AprilTagDetector(H, W, max_batch=n)}
    out = {}
    for fourcc in R.FAMILIES:
        stride = R.min_stride(fourcc, W)
        src = torch.randint(0, 256, (n * H * stride,), dtype=torch.uint8, device="cuda")
        moved = n * H * (stride + W)                       # bytes read + written
        a = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        b = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for o in R.ORIENTATIONS:
            det = dets[(H, W)] if o in ("clockwise", "counterclockwise") else dets[(W, H)]
            ts = []
            for rep in range(5):
                t0 = time.perf_counter()
                det.upload_raw_device(src.data_ptr(), n, stride, H * stride, fourcc, o)
                ts.append(time.perf_counter() - t0)
            out[f"{fourcc}/{o}"] = {"bytes_moved": moved, "call_ms_min": round(min(ts) * 1e3, 3)}
        for rep in range(5):
            b.copy_(a)                                     # hipMemcpyAsync device-to-device: reads moved/2, writes moved/2
        torch.cuda.synchronize()
        out[f"{fourcc}/copy"] = {"bytes_moved": moved}
    for d in dets.values():
        d.close()
    return {"mode": "kernels", "frames": n, "size": [W, H], "cases": out}


def calls(n):
    from chalkydri_amd.detector import AprilTagDetector
    det = AprilTagDetector(W, H, max_batch=n)
    rng = np.random.default_rng(0)
    out = {}
    for fourcc in ("YUYV", "RGB3"):
        stride = R.min_stride(fourcc, W)
        raw = rng.integers(0, 256, (n, H, stride), dtype=np.uint8)          # pageable
        luma = np.empty((n, H, W), np.uint8)

        def host_convert(i):
            luma[i] = R.luma_vec(raw[i], fourcc, W, H, stride)              # numpy releases the GIL in its inner loops

        res = {}
        for name in ("upload_raw", "host16_then_upload_frames"):
            wall, cpu = [], []
            for rep in range(4):
                t0, c0 = time.perf_counter(), time.process_time()
                if name == "upload_raw":
                    det.upload_raw(raw, fourcc)
                else:
                    with ThreadPoolExecutor(16) as ex:
                        list(ex.map(host_convert, range(n)))
                    det.upload(luma)
                wall.append(time.perf_counter() - t0); cpu.append(time.process_time() - c0)
            res[name] = {"wall_ms_min": round(min(wall[1:]) * 1e3, 2), "cpu_s_min": round(min(cpu[1:]), 3)}
        assert np.array_equal(det.raw_luma(raw[:2], fourcc), np.stack([R.luma_vec(raw[i], fourcc, W, H, stride) for i in range(2)]))
        out[fourcc] = res
    det.close()
    return {"mode": "calls", "frames": n, "size": [W, H], "cases": out}


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "calls"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    print(json.dumps(kernels(n) if mode == "kernels" else calls(n)))
