"""Per-tag pose on the MI355X (ck_estimate_tag_poses / ck_last_tag_poses, k_tagpose.hip): against the numpy restatement
(tests/np_tag_pose.py) on the GPU's own detections, against the rendered truth, the two entry points against each other, tag
sizes and families, degenerate input and errors, and that nothing else the handle computes changes."""
import ctypes as C
import math

import numpy as np
import pytest

import np_tag_pose as T
import tag_pose_util as U
from chalkydri_amd import _abi as A
from chalkydri_amd import scenes, synth
from chalkydri_amd.apriltags import AprilTags
from chalkydri_amd.detector import AprilTagDetector, IngestRing, _raw_detections, tag_pose_params

pytestmark = pytest.mark.gpu


def _cam(w, h, f=None):
    f = float(w) if f is None else f
    return (f, f, w / 2.0, h / 2.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def _params(cam, tagsize=0.1651, n_iters=50):
    return tag_pose_params(*cam[:4], tagsize=tagsize, distortion=cam[4:], n_iters=n_iters)


def _flat_raw(dets_per_frame):
    arr, n = _raw_detections([d for fr in dets_per_frame for d in fr])
    return arr, n


@pytest.mark.parametrize("fam,dec,w,h,nf", [("tag36h11", 1, 640, 480, 4), ("tag16h5", 2, 1280, 800, 3),
                                            ("tag36h11", 2, 320, 240, 4), ("tag16h5", 1, 320, 240, 4),
                                            ("tag36h11", 2, 640, 480, 256)])
def test_gpu_matches_restatement(built, fam, dec, w, h, nf):
    frames, _ = synth.render_batch(7, nf, w, h, 6, families=(fam,))
    det = AprilTagDetector(w, h, max_batch=nf, families=(fam,), quad_decimate=dec)
    dets = det.detect_batch(frames, cap=64)
    arr, n = _flat_raw(dets)
    assert n > 0
    cam = _cam(w, h)
    gpu = U.records_of(det.estimate_tag_poses(arr[:n], _params(cam), raw=True))
    ref, infos = U.np_poses(arr[:n], cam, [0.1651])
    stats = {}
    bad = U.compare(gpu, ref, infos, stats)
    print(f"\n{fam} dec {dec} {w}x{h}x{nf}: {stats}")
    assert not bad, bad[:5]
    assert sum(g["valid"] for g in gpu) == n


def test_gpu_pose_against_truth(built):
    rows = []
    for (fam, dec, w, h) in [("tag36h11", 2, 640, 480), ("tag36h11", 1, 1280, 800), ("tag16h5", 1, 320, 240), ("tag16h5", 2, 1280, 800)]:
        frames, truths = synth.render_batch(11, 12, w, h, 6, families=(fam,))
        det = AprilTagDetector(w, h, max_batch=12, families=(fam,), quad_decimate=dec)
        dets = det.detect_batch(frames)
        poses = det.last_tag_poses(_params(_cam(w, h)), raw=True)
        for fd, fp, tr in zip(dets, poses, truths):
            for d, p in zip(fd, U.records_of(fp)):
                m = U.match_synth(d.corners(), d.id(), tr)
                if m is None:
                    continue
                R, t = U.synth_truth(m["H"], w, h, 0.1651)
                rows.append(U.truth_errors(p, R, t))
    e = np.array(rows)
    print(f"\nsynth truth: n={len(e)} rot median {np.median(e[:, 0]):.3f} p90 {np.percentile(e[:, 0], 90):.3f} "
          f"best max {e[:, 1].max():.3f} t_rel max {e[:, 2].max():.4f}")
    assert len(e) > 100
    assert np.median(e[:, 0]) <= U.TRUTH_ROT_MEDIAN_DEG and np.percentile(e[:, 0], 90) <= U.TRUTH_ROT_P90_DEG
    assert e[:, 1].max() <= U.TRUTH_ROT_BEST_DEG and e[:, 2].max() <= U.TRUTH_T_REL
    # scenes.render_view: the field wall seen from the robot
    w, h, f = 1280, 800, 800.0
    layout = scenes.wall_layout(6)
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
    rng = np.random.default_rng(5)
    det = AprilTagDetector(w, h, max_batch=1)
    rows = []
    for i in range(8):
        pose = (rng.uniform(0.6, 3.6), rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3))
        frame, _ = scenes.render_view(77 + i, w, h, f, layout, pose, r2c)
        truth = U.view_truths(layout, pose, r2c)
        fd = det.detect(frame)
        for d, p in zip(fd, U.records_of(det.last_tag_poses(_params(_cam(w, h, f)), raw=True)[0])):
            rows.append(U.truth_errors(p, *truth[d.id()]))
    e = np.array(rows)
    print(f"view truth: n={len(e)} best max {e[:, 1].max():.3f} t_rel max {e[:, 2].max():.4f}")
    assert len(e) > 20 and e[:, 1].max() <= U.TRUTH_ROT_BEST_DEG and e[:, 2].max() <= U.TRUTH_T_REL


def _bytes(recs):
    return b"".join(bytes(r) for r in recs)


def test_two_entry_points_one_answer(built):
    import torch
    w, h, nf = 640, 480, 4
    frames, _ = synth.render_batch(3, nf, w, h, 6)
    det = AprilTagDetector(w, h, max_batch=nf)
    pp = _params(_cam(w, h))
    # before any detect call: nothing to read
    counts = (C.c_int32 * nf)()
    out = (A.TagPose * (nf * 8))()
    assert det._L.ck_last_tag_poses(det._h, C.byref(pp), out, 8, counts) == A.CK_EINVAL

    def check_against(dets, cap=64):
        last = det.last_tag_poses(pp, cap=cap, raw=True)
        assert len(last) == len(dets)
        for fd, fl in zip(dets, last):
            assert len(fl) == min(len(fd), cap)
            arr, n = _raw_detections(fd[:cap])
            if n:
                assert _bytes(fl) == _bytes(det.estimate_tag_poses(arr[:n], pp, raw=True))
        return last

    d1 = det.detect_batch(frames)
    assert sum(len(x) for x in d1) > 8
    first = check_against(d1)
    check_against(d1, cap=2)                                     # the cap_per_frame truncation
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    d2, _ = det.detect_device(dev.data_ptr(), nf, w, w * h)
    assert _bytes(sum(check_against(d2), [])) == _bytes(sum(first, []))
    ring = IngestRing(det, n_slots=1)
    for i in range(nf):
        ring.write(0, i, frames[i])
    ring.submit(0, nf)
    d3, _ = ring.detect(0, nf)
    assert _bytes(sum(check_against(d3), [])) == _bytes(sum(first, []))
    ring.close()
    det.upload(frames)
    pr = A.ProcessParams()
    pr.cam = A.OpenCV5(*_cam(w, h))
    det._L.ck_sqpnp_params_default(C.byref(pr.sqpnp))
    g, hg = np.zeros(nf), np.zeros(nf, np.uint8)
    meas, valid = (A.VisionMeasurement * nf)(), (C.c_int32 * nf)()
    assert det._L.ck_process_uploaded(det._h, nf, C.byref(pr), g.ctypes.data, hg.ctypes.data, meas, valid) == 0
    assert _bytes(sum(check_against(d1), [])) == _bytes(sum(first, []))
    # a stage call that rewrites the workspace ends it; a plain upload does not
    det.upload(frames)
    assert _bytes(sum(det.last_tag_poses(pp, raw=True), [])) == _bytes(sum(first, []))
    det.quads(frames)
    assert det._L.ck_last_tag_poses(det._h, C.byref(pp), out, 8, counts) == A.CK_EINVAL
    det.detect_batch(frames[:2])
    assert len(det.last_tag_poses(pp)) == 2


def test_families_and_tag_sizes(built):
    fams = ("tag36h11", "tag16h5", "tag36h11", "tag16h5")
    det = AprilTagDetector(320, 240, max_batch=1, families=fams)
    sizes = [0.1651, 0.05, 0.3, 0.12]
    cam = (600.0, 610.0, 160.0, 120.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    rng = np.random.default_rng(2)
    recs, truth = [], []
    for k in range(64):
        fam = k % 4
        R, t = U.random_pose(rng, 0.5, 4.0)
        c = U.project(R, t, sizes[fam] / 2, cam)
        d = A.Detection()
        d.id, d.family = k, fam
        for i in range(4):
            d.p[i][0], d.p[i][1] = c[i]
        recs.append(d)
        truth.append((R, t))
    arr, n = _raw_detections(recs)
    base = det.estimate_tag_poses(arr, _params(cam, sizes), raw=True)
    dbl = det.estimate_tag_poses(arr, _params(cam, [2 * s for s in sizes]), raw=True)
    for r, r2, (R, t) in zip(base, dbl, truth):
        assert r.valid and r2.valid and r.has_alt == r2.has_alt
        best = min(np.abs(np.array(r.t[:]) - t).max(), np.abs(np.array(r.t_alt[:]) - t).max() if r.has_alt else 9)
        assert best < 1e-6 * max(1.0, np.linalg.norm(t))
        assert bytes(r.R) == bytes(r2.R) and bytes(r.R_alt) == bytes(r2.R_alt) and bytes(r.H) == bytes(r2.H)
        assert all(2 * a == b for a, b in zip(r.t[:], r2.t[:])) and all(2 * a == b for a, b in zip(r.t_alt[:], r2.t_alt[:]))
        assert 4 * r.err == r2.err and (4 * r.err_alt == r2.err_alt)


def test_degenerate_and_invalid_input(built):
    det = AprilTagDetector(320, 240, max_batch=1)
    cam = (600.0, 600.0, 160.0, 120.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    pp = _params(cam)
    R, t = U.rot([1, 0.3, 0], 0.4), np.array([0.1, -0.05, 1.5])
    good = U.project(R, t, 0.1651 / 2, cam)
    cases = {"coincident": np.full((4, 2), 100.0), "collinear": np.array([[10.0, 10], [20, 20], [30, 30], [40, 40]]),
             "three collinear": np.array([[10.0, 10], [20, 20], [30, 30], [10, 40]]),
             "nan corner": np.where(np.arange(8).reshape(4, 2) == 3, np.nan, good), "inf corner": good + [[np.inf, 0], [0, 0], [0, 0], [0, 0]]}
    recs = []
    for k, c in enumerate(cases.values()):
        d = A.Detection()
        d.id, d.family = k, 0
        for i in range(4):
            d.p[i][0], d.p[i][1] = c[i]
        recs.append(d)
    for fam in (-1, 1, 7):   # families outside the handle's one
        d = A.Detection()
        d.id, d.family = 99, fam
        for i in range(4):
            d.p[i][0], d.p[i][1] = good[i]
        recs.append(d)
    arr, n = _raw_detections(recs)
    out = det.estimate_tag_poses(arr, pp, raw=True)
    for r, d in zip(out, recs):
        v = np.array(r.R[:] + r.t[:] + r.R_alt[:] + r.t_alt[:] + r.H[:] + [r.err, r.err_alt])
        assert r.valid == 0 and r.has_alt == 0 and not v.any() and (r.id, r.family) == (d.id, d.family), (d.id, d.family)
    # a tag behind the camera projects to the same corners as the tag in front turned by pi about its normal: a valid pose
    Rb, tb = R, -t
    P = T.object_points(0.1651 / 2) @ Rb.T + tb
    behind = np.stack([600 * P[:, 0] / P[:, 2] + 160, 600 * P[:, 1] / P[:, 2] + 120], 1)
    d = A.Detection()
    for i in range(4):
        d.p[i][0], d.p[i][1] = behind[i]
    arr, _ = _raw_detections([d])
    r = det.estimate_tag_poses(arr, _params(cam, n_iters=1000), raw=True)[0]
    front = (R @ U.rot([0, 0, 1], math.pi), t)
    assert r.valid and r.t[2] > 0 and np.all(np.isfinite(r.R[:]))
    sols = [(np.array(r.R[:]).reshape(3, 3), np.array(r.t[:]))] + ([(np.array(r.R_alt[:]).reshape(3, 3), np.array(r.t_alt[:]))] if r.has_alt else [])
    assert min(max(np.abs(a - front[0]).max(), np.abs(b - front[1]).max()) for a, b in sols) < 1e-8
    # parameter errors, capacity
    L, h = det._L, det._h
    arr, n = _raw_detections(recs[:1])
    o = (A.TagPose * 1)()

    def rc(p, dets=arr, cnt=1, dst=o):
        return L.ck_estimate_tag_poses(h, C.byref(p), dets, cnt, dst)
    assert rc(pp) == 0
    for field, val in [("fx", 0.0), ("fy", -1.0), ("fx", math.nan), ("fy", math.inf), ("cx", math.inf), ("cy", math.nan),
                       ("k1", math.nan), ("k2", math.inf), ("p1", math.nan), ("p2", math.nan), ("k3", math.inf)]:
        bad = _params(cam)
        setattr(bad.cam, field, val)
        assert rc(bad) == A.CK_EINVAL, field
    for ts in (0.0, -0.1, math.nan, math.inf):
        assert rc(_params(cam, [ts, 0.1651, 0.1651, 0.1651])) == A.CK_EINVAL
    assert rc(_params(cam, [0.1651, 0.0, math.nan, -1.0])) == 0   # families the handle does not have are not checked
    for it in (0, -1, 1001):
        assert rc(_params(cam, n_iters=it)) == A.CK_EINVAL
    assert rc(_params(cam, n_iters=1000)) == 0 and rc(_params(cam, n_iters=1)) == 0
    assert L.ck_estimate_tag_poses(h, None, arr, 1, o) == A.CK_EINVAL
    assert L.ck_estimate_tag_poses(h, C.byref(pp), None, 1, o) == A.CK_EINVAL
    assert L.ck_estimate_tag_poses(h, C.byref(pp), arr, 1, None) == A.CK_EINVAL
    assert L.ck_estimate_tag_poses(h, C.byref(pp), arr, -1, o) == A.CK_EINVAL
    assert L.ck_estimate_tag_poses(None, C.byref(pp), arr, 1, o) == A.CK_EINVAL
    big = (A.Detection * 257)()
    bigo = (A.TagPose * 257)()
    assert L.ck_estimate_tag_poses(h, C.byref(pp), big, 257, bigo) == A.CK_ECAPACITY
    assert L.ck_estimate_tag_poses(h, C.byref(pp), big, 256, bigo) == 0
    cnt = (C.c_int32 * 1)()
    assert L.ck_last_tag_poses(h, C.byref(pp), bigo, 0, cnt) == A.CK_EINVAL
    assert L.ck_last_tag_poses(h, C.byref(pp), None, 4, cnt) == A.CK_EINVAL


def test_nothing_else_changes(built):
    w, h, nf = 640, 480, 4
    frames, gyro, layout, calib, r2c = scenes.bench_stream(1, nf, w, h, 6)
    task = AprilTags(w, h, layout, calib, r2c, cam_id=1, max_batch=nf)
    det = task.detector
    c = calib["OpenCVModel5"]
    pp = tag_pose_params(c["fx"], c["fy"], c["cx"], c["cy"])
    d0 = det.detect_batch(frames)
    m0, v0 = task.process_batch(frames, list(gyro))
    p1 = det.last_tag_poses(pp, raw=True)
    d1 = det.detect_batch(frames)
    p2 = det.last_tag_poses(pp, raw=True)
    arr, n = _flat_raw(d1)
    e1 = det.estimate_tag_poses(arr[:n], pp, raw=True)
    e2 = det.estimate_tag_poses(arr[:n], pp, raw=True)
    m1, v1 = task.process_batch(frames, list(gyro))
    key = lambda ds: [(d.id(), d.corners().tobytes(), d.center().tobytes(), d.decision_margin()) for fr in ds for d in fr]
    assert key(d0) == key(d1)
    assert bytes(m0) == bytes(m1) and list(v0) == list(v1)
    assert _bytes(sum(p1, [])) == _bytes(sum(p2, [])) == _bytes(e1) == _bytes(e2)
    assert sum(r.valid for r in e1) == n > 0
