#!/usr/bin/env python3
"""Times the camera rig for 256 steps x 3 cameras x 4 tags: ck_rig_process_last on three handles whose ck_process_* call
of 256 rendered frames each has just run (three cameras 0.3 m apart on one robot, a wall of 4 tags), beside the three k_sqpnp launches
the per-camera path pays for the same frames, both between hipEvents on handles[0]'s stream (ck_rig_time_last: gyro in, kernel,
records out; the k_sqpnp launches back to back), 3 warm-ups, the median of --reps runs; and ck_rig_solve_host, one thread, on packed
synthetic rigs of the same shape (the C call alone is timed).  Then the accuracy on the end-to-end scene of tests/test_gpu_rig.py (two
cameras at yaw +-25 degrees, 0.3 m apart, a wall of 12 tags) from 100 robot poses with noisy bearings: the RMS position error of the
fused pose beside each single camera's.  One JSON line.

  python tools/bench_rig.py [--reps 20] [--warmup 3] [--steps 256] [--noise 1e-3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import np_rig as N  # noqa: E402
from chalkydri_amd import scenes  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd._lib import check  # noqa: E402
from chalkydri_amd.apriltags import AprilTags  # noqa: E402
from chalkydri_amd.rig import RESULT_DTYPE, RigSolver, pack_steps  # noqa: E402
from chalkydri_amd.sqpnp import SqPnP, iso3  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def to_step(cams):
    return [([iso3(t, N.mat_to_quat(R)) for R, t in tags], b, iso3(bb, N.mat_to_quat(Am))) for tags, b, (Am, bb) in cams]


def wall_scene(rng, noise):
    """The end-to-end scene with synthetic bearings: the tags of the wall each camera has in its field of view"""
    layout = scenes.wall_layout(12)
    mounts = [scenes.solver_camera_transform(0.2, y, 0.6, 0.0, 0.0, yaw) for y, yaw in ((0.15, 25.0), (-0.15, -25.0))]
    half = (np.arctan(320 / 550.0), np.arctan(400 / 700.0))
    x, y, yaw = rng.uniform(1.5, 2.5), rng.uniform(-0.6, 0.6), rng.uniform(-0.25, 0.25)
    Rwr, twr = N.rot_z(yaw), np.array([x, y, 0.0])
    cams = []
    for (Am, bb), fov in zip(mounts, half):
        tags, bearings = [], []
        for t in layout["tags"]:
            tr, q = t["pose"]["translation"], t["pose"]["rotation"]["quaternion"]
            Rt, tt = N.quat_to_mat([q["W"], q["X"], q["Y"], q["Z"]]), np.array([tr["x"], tr["y"], tr["z"]])
            pc = ((Rt @ N.CORNERS.T).T + tt - twr) @ Rwr @ Am.T + bb
            if pc[:, 2].min() < 0.3 or np.abs(np.arctan2(pc[:, 0], pc[:, 2])).max() > fov:
                continue
            xy = pc[:, :2] / pc[:, 2:3] + rng.normal(0, noise, (4, 2))
            v = np.concatenate([xy, np.ones((4, 1))], 1)
            tags.append((Rt, tt)); bearings.append(v / np.linalg.norm(v, axis=1, keepdims=True))
        cams.append((tags, np.concatenate(bearings) if bearings else np.zeros((0, 3)), (Am, bb)))
    return cams, yaw + rng.normal(0, 0.02), twr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--noise", type=float, default=1e-3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    out = {"steps": a.steps, "cameras": 3, "tags_per_camera": 4, "reps": a.reps, "warmup": a.warmup}
    # device: three tasks process the rendered frames of one robot, then the fusion and the three k_sqpnp launches between events
    w, h, f, unique = 640, 480, 600.0, 8
    layout = scenes.wall_layout(4)
    mounts = [{"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": y, "z": 0.6} for y in (0.3, 0.0, -0.3)]
    tasks = [AprilTags(w, h, layout, scenes.pinhole_calib(f, w / 2.0, h / 2.0), m, cam_id=c, max_batch=a.steps) for c, m in enumerate(mounts)]
    poses = [(rng.uniform(1.0, 1.6), rng.uniform(-0.2, 0.2), rng.uniform(-0.05, 0.05)) for _ in range(unique)]
    gyro = np.array([poses[i % unique][2] for i in range(a.steps)])
    has = np.ones(a.steps, np.uint8)
    seen = []
    for c, t in enumerate(tasks):
        frames = np.stack([scenes.render_view(100 + 10 * i + c, w, h, f, layout, p, mounts[c], noise_amp=1)[0] for i, p in enumerate(poses)])
        recs, valid = t.process_batch(frames[np.arange(a.steps) % unique], list(gyro))
        seen.append(float(np.mean([r.tag_count for r in recs])))
    L = tasks[0].detector._L
    prm = RigSolver(rig_id=200).params
    hs = (C.c_void_p * 3)(*[t.detector._h.value for t in tasks])
    iters = a.warmup + a.reps
    ms_rig, ms_sq = np.zeros(iters, np.float32), np.zeros(iters, np.float32)
    check(L.ck_rig_time_last(hs, 3, a.steps, C.byref(prm), gyro.ctypes.data, has.ctypes.data, iters, ms_rig.ctypes.data, ms_sq.ctypes.data), "ck_rig_time_last")
    res = np.zeros(a.steps, RESULT_DTYPE)
    meas, valid = (A.VisionMeasurement * a.steps)(), (C.c_int32 * a.steps)()
    check(L.ck_rig_process_last(hs, 3, a.steps, C.byref(prm), gyro.ctypes.data, has.ctypes.data, res.ctypes.data_as(C.POINTER(A.RigResult)), meas, valid),
          "ck_rig_process_last")
    stat = lambda v: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
    out["rig_process_last_device"] = stat(ms_rig[a.warmup:])
    out["three_k_sqpnp_device"] = stat(ms_sq[a.warmup:])
    out["three_k_sqpnp_over_rig"] = out["three_k_sqpnp_device"]["median_ms"] / out["rig_process_last_device"]["median_ms"]
    out["detections_per_camera"] = seen
    out["rig_valid"] = int(np.sum(valid[:]))
    out["rig_tags_per_step"] = float(res["n_tags"].mean())
    for t in tasks:
        t.detector.close()
    # host twin, one thread: synthetic rigs of the same shape, packed outside the timed call
    steps, gyros = [], []
    for _ in range(a.steps):
        cams, g, _ = N.make_rig(rng, n_cams=3, noise=a.noise, tags_per_cam=(4, 4), gyro_noise=0.02)
        steps.append(to_step(cams)); gyros.append(g)
    n_cams, probs, tarr, nt, barr = pack_steps(steps)
    garr, hres = np.array(gyros), np.zeros(a.steps, RESULT_DTYPE)
    out["rig_host_one_thread"] = timed(lambda: check(L.ck_rig_solve_host(C.byref(prm), n_cams, probs, a.steps, tarr, nt, barr.ctypes.data, len(barr),
                                                                         garr.ctypes.data, hres.ctypes.data_as(C.POINTER(A.RigResult))), "ck_rig_solve_host"),
                                       max(3, a.reps // 4), 1)
    out["host_over_device"] = out["rig_host_one_thread"]["median_ms"] / out["rig_process_last_device"]["median_ms"]
    det = AprilTagDetector(64, 64)
    rig, single = RigSolver(det), SqPnP(det)
    # accuracy: the fused pose beside each camera alone
    scene = [wall_scene(rng, a.noise) for _ in range(100)]
    scene = [s for s in scene if all(len(c[0]) for c in s[0])]
    fused = rig.solve_batch([to_step(c) for c, _, _ in scene], [g for _, g, _ in scene])
    err = {"fused": [], "cam0": [], "cam1": []}
    alone = [single.solve_batch([(st[c][0], st[c][1], st[c][2], g, 600.0) for st, g in ((to_step(cams), g) for cams, g, _ in scene)]) for c in range(2)]
    for i, (_, _, twr) in enumerate(scene):
        if fused[i]["valid"] and alone[0][i] is not None and alone[1][i] is not None:
            err["fused"].append(np.linalg.norm(fused[i]["pos"][:2] - twr[:2]))
            for c in range(2):
                err["cam%d" % c].append(np.linalg.norm(alone[c][i]["pos"][:2] - twr[:2]))
    out["accuracy"] = {"poses": len(err["fused"]), "bearing_noise": a.noise,
                       **{"rms_pos_err_m_" + k: float(np.sqrt(np.mean(np.square(v)))) for k, v in err.items()}}
    out["accuracy"]["rms_pos_err_m_better_single"] = min(out["accuracy"]["rms_pos_err_m_cam0"], out["accuracy"]["rms_pos_err_m_cam1"])
    det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
