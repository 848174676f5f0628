#!/usr/bin/env python3
"""Times the sub-pixel corner calls (ck_subpix.hip) on the device against their one-thread host twins, and the detector
setting inside the bench.py workload.  Prints one JSON line per measurement:

  corner_subpix   256 frames x 24 corners (6144 points; four rendered AprilGrid views, repeated) through ck_corner_subpix with every
                  array on the device, against ck_corner_subpix_host on one thread, and the bytes compared
  board_corners   ck_board_corners_last for 64 board frames (the same views) against ck_board_corners_host on one thread
  setting         bench.py's default workload (256 distinct 1280 x 800 frames, 6 tags, detect + pose) with the setting off and on,
                  alternating: milliseconds per step, and the decode stage between its events, which holds the extra kernel

Times are host clocks around calls that end in a synchronise of the handle's stream; median and minimum over --iters calls after one
warm call.  Run it alone, and under `rocprofv3 --kernel-trace --stats -- python tools/bench_subpix.py --only corner_subpix` for the
kernel time itself.
usage: python tools/bench_subpix.py [--iters N] [--only NAME]"""
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

import subpix_scenes as SC  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd import scenes, subpix  # noqa: E402
from chalkydri_amd.apriltags import AprilTags  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402


def timed(call, iters):
    call()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


def views():
    return np.stack([SC.board_frame(s, 0.8)[0] for s in SC.SEEDS]), [SC.board_frame(s, 0.8)[1]["uv"] for s in SC.SEEDS]


def bench_corner_subpix(iters):
    frames4, truth = views()
    n_frames, per = 256, 24
    det = AprilTagDetector(SC.W, SC.H, max_batch=n_frames)
    det.upload(frames4[np.arange(n_frames) % 4])
    rng = np.random.default_rng(1)
    fr = np.repeat(np.arange(n_frames, dtype=np.int32), per)
    xy = np.concatenate([truth[f % 4].reshape(-1, 2)[rng.choice(64, per, replace=False)] for f in range(n_frames)]) + rng.uniform(-1, 1, (n_frames * per, 2))
    n = len(xy)
    pp = subpix.subpix_params()
    d_fr, d_xy = torch.from_numpy(fr).cuda(), torch.from_numpy(xy).cuda()
    d_out, d_info = torch.zeros((n, 2), dtype=torch.float64, device="cuda"), torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call():
        assert det._L.ck_corner_subpix(det._h, C.byref(pp), C.c_void_p(d_fr.data_ptr()), C.c_void_p(d_xy.data_ptr()), n, C.c_void_p(d_out.data_ptr()),
                                       C.c_void_p(d_info.data_ptr())) == 0
    med, best = timed(call, iters)
    t0 = time.perf_counter()
    want, info = subpix.corner_subpix_host(frames4, fr % 4, xy, pp, return_info=True)
    host_ms = (time.perf_counter() - t0) * 1e3
    same = d_out.cpu().numpy().tobytes() == want.tobytes() and d_info.cpu().numpy().tobytes() == info.tobytes()
    print(json.dumps({"what": "corner_subpix", "points": n, "half_win": pp.half_win, "device_median_ms": med, "device_min_ms": best,
                      "host_one_thread_ms": round(host_ms, 2), "mean_iters": round(float(info["iters"].mean()), 2),
                      "converged": int((info["status"] == A.CK_SUBPIX_CONVERGED).sum()), "bytes_equal": bool(same), "iters": iters}), flush=True)
    det.close()


def bench_board_corners(iters):
    frames4, _ = views()
    n_frames = 64
    frames = frames4[np.arange(n_frames) % 4]
    det = AprilTagDetector(SC.W, SC.H, max_batch=n_frames)
    dets = det.detect_batch(frames)
    board = SC.board()
    out = {}

    def call():
        out["uv"], out["state"] = det.board_corners(board)
    med, best = timed(call, iters)
    t0 = time.perf_counter()
    wuv, wstate = subpix.board_corners_host(board, frames, dets)
    host_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"what": "board_corners", "frames": n_frames, "tags_per_frame": 16, "seeds": int((wstate == 1).sum()), "known": int((wstate > 0).sum()),
                      "device_median_ms": med, "device_min_ms": best, "host_one_thread_ms": round(host_ms, 2),
                      "bytes_equal": bool(out["uv"].tobytes() == wuv.tobytes() and out["state"].tobytes() == wstate.tobytes()), "iters": iters}), flush=True)
    det.close()


def bench_setting(iters):
    w, h, n = 1280, 800, 256
    frames, gyro, layout, calib, r2c = scenes.bench_stream(2, n, w, h, 6, stream=0, unique=n, noise_amp=3)
    task = AprilTags(w, h, layout, calib, r2c, cam_id=0, max_batch=n)
    det = task.detector
    det.upload(frames)
    d_gyro = torch.from_numpy(np.ascontiguousarray(gyro)).cuda()
    d_has = torch.ones(n, dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    d_valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    step = lambda: task.process_uploaded_into(n, d_gyro.data_ptr(), d_has.data_ptr(), d_rec.data_ptr(), d_valid.data_ptr())  # noqa: E731
    res = {False: {"step": [], "decode": []}, True: {"step": [], "decode": []}}
    n_dets = sum(len(f) for f in det.detect_batch(n=n))
    for on in (False, True):  # warm both
        det.set_corner_subpix(on=on)
        step()
    for _ in range(iters):
        for on in (False, True):
            det.set_corner_subpix(on=on)
            t0 = time.perf_counter()
            step()
            res[on]["step"].append((time.perf_counter() - t0) * 1e3)
            res[on]["decode"].append(det.stage_ms()["decode"])
    valid_on = int(d_valid.cpu().numpy().sum())
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    print(json.dumps({"what": "setting", "frames": n, "detections": n_dets, "corners_refined": 4 * n_dets, "valid_poses_on": valid_on,
                      "off_ms_per_step": med(res[False]["step"]), "on_ms_per_step": med(res[True]["step"]),
                      "off_decode_ms": med(res[False]["decode"]), "on_decode_ms": med(res[True]["decode"]),
                      "extra_between_events_ms": round(med(res[True]["decode"]) - med(res[False]["decode"]), 4),
                      "off_spread_ms": [round(float(np.min(res[False]["step"])), 4), round(float(np.max(res[False]["step"])), 4)], "iters": iters}), flush=True)
    det.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=("corner_subpix", "board_corners", "setting"), default=None)
    args = ap.parse_args()
    torch.cuda.init()
    for name, fn in (("corner_subpix", bench_corner_subpix), ("board_corners", bench_board_corners), ("setting", bench_setting)):
        if args.only in (None, name):
            fn(args.iters)


if __name__ == "__main__":
    main()
