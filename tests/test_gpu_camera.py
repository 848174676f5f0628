"""Camera models on the MI355X (ck_camera_unproject, ck_set_camera): the device unprojection returns the host twin's
bytes for every model; a handle with EUCM alpha = 0 set returns the bytes of the zero-distortion OpenCVModel5 path; the bearings the
glue leaves in the workspace are the host twin's of the known detections' corners; a pinhole scene resampled through an EUCM lens gives
the pose back with the EUCM model and a worse one with the pinhole; misuse."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_camera as NC  # noqa: E402
import scenes  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, F = 640, 480, 576.0
R2C = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
POSE = (2.2, 0.1, 0.05)


@pytest.fixture(scope="module")
def scene(built):
    """One 640 x 480 frame of a wall of six tags (the scene of test_gpu_pose.py's small cases), rendered once."""
    layout = scenes.wall_layout(6, cols=3)
    frame, truth = scenes.render_view(71, W, H, F, layout, POSE, R2C, noise_amp=1)
    return {"layout": layout, "frame": frame, "truth": truth, "calib": scenes.pinhole_calib(F, W / 2.0, H / 2.0)}


def _task(scene, calib, max_batch=1):
    from chalkydri_amd.apriltags import AprilTags
    return AprilTags(W, H, scene["layout"], calib, R2C, cam_id=3, max_batch=max_batch)


def _bytes(recs):
    return b"".join(bytes(r) for r in recs)


def _pose_bytes(poses):
    return b"".join(bytes(p) for fr in poses for p in fr)


def _farthest(dets):
    """(index, r2) of the detection whose centre is farthest from the principal point, r2 in normalised units."""
    r2 = [((d.center()[0] - W / 2.0) / F) ** 2 + ((d.center()[1] - H / 2.0) / F) ** 2 for d in dets]
    return int(np.argmax(r2)), float(max(r2))


@pytest.mark.parametrize("n", [1, 127, 128, 129, 4097])
def test_device_unprojection_returns_the_host_bytes(built, n):
    """Blocks of 128 threads: one point, one short of a block, a block, one more, many blocks and a tail.  A fifth of the pixels lie
    far outside the image: outside EUCM's valid disc, and where OpenCVModel5's iteration does not converge."""
    from chalkydri_amd import camera
    from chalkydri_amd.sqpnp import unproject_opencv5
    rng = np.random.default_rng(n)
    px = rng.uniform(0, 1, (n, 2)) * [NC.W, NC.H]
    far = rng.uniform(0, 1, n) < 0.2
    px[far] = rng.uniform(-6000, 7000, (int(far.sum()), 2))
    if n == 1:
        px = np.array([[3000.0, 400.0]])                                   # outside the wide lens' disc (r = 982 px)
    k5 = (900.0, 905.0, 640.0, 400.0, -0.28, 0.07, 1e-3, -2e-4, 0.01)
    cams = [camera.make_camera("EUCM", *NC.LENSES["eucm_wide"]), camera.make_camera("UCM", *NC.LENSES["ucm"][:5]),
            camera.make_camera("EUCM", *NC.LENSES["eucm_mild"]), camera.make_camera("OpenCVModel5", *k5)]
    for c in cams:
        bh, okh = camera.unproject_host(c, px)
        bd, okd = camera.unproject(c, px)
        assert bd.tobytes() == bh.tobytes() and np.array_equal(okd, okh), c.model
        if c is cams[0] or (n > 1 and c.model == A.CK_CAMERA_OPENCV5):
            assert not okh.all()                                           # the invalid ones are really among them
        assert n == 1 or okh.any()
    b5, ok5 = unproject_opencv5(k5, px)
    assert b5.tobytes() == bd.tobytes() and np.array_equal(ok5, okd)       # (bd: the OpenCVModel5 camera, the last of the loop)


def test_alpha_zero_camera_returns_the_pinhole_path_bytes(scene):
    """ck_process_uploaded and ck_last_tag_poses after ck_set_camera(EUCM, alpha = 0) = the zero-distortion OpenCVModel5 params without
    it, byte for byte; ck_set_camera(NULL) then gives, for a distorted OpenCVModel5, the bytes of a handle that never had a camera set."""
    from chalkydri_amd import camera
    from chalkydri_amd.detector import tag_pose_params
    task = _task(scene, scene["calib"])
    det = task.detector
    tp = tag_pose_params(F, F, W / 2.0, H / 2.0)
    recs0, valid0 = task.process_batch(scene["frame"][None], [POSE[2]])
    poses0 = det.last_tag_poses(tp, raw=True)
    assert valid0.all() and recs0[0].tag_count >= 2 and len(poses0[0]) == recs0[0].tag_count and all(p.valid for p in poses0[0])
    det.set_camera(camera.make_camera("EUCM", F, F, W / 2.0, H / 2.0, 0.0, 1.08))
    task._pp.cam = A.OpenCV5(1.0, 1.0, 0.0, 0.0, 9.0, 9.0, 9.0, 9.0, 9.0)     # ignored while a camera is set
    tp_junk = tag_pose_params(1.0, 1.0, 0.0, 0.0, distortion=(9.0,) * 5)
    recs1, valid1 = task.process_batch(scene["frame"][None], [POSE[2]])
    assert _bytes(recs1) == _bytes(recs0) and np.array_equal(valid1, valid0)
    assert _pose_bytes(det.last_tag_poses(tp_junk, raw=True)) == _pose_bytes(poses0)
    # back to the params' model, now a distorted one; the other handle never had a camera
    det.set_camera(None)
    m = scenes.REF_CALIB["OpenCVModel5"]
    dist = A.OpenCV5(F, F, W / 2.0, H / 2.0, *(m[k] for k in ("k1", "k2", "p1", "p2", "k3")))
    tpd = tag_pose_params(F, F, W / 2.0, H / 2.0, distortion=[m[k] for k in ("k1", "k2", "p1", "p2", "k3")])
    task._pp.cam = dist
    recs2, valid2 = task.process_batch(scene["frame"][None], [POSE[2]])
    poses2 = det.last_tag_poses(tpd, raw=True)
    fresh = _task(scene, {"OpenCVModel5": {f: getattr(dist, f) for f in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")}})
    recs3, valid3 = fresh.process_batch(scene["frame"][None], [POSE[2]])
    assert _bytes(recs2) == _bytes(recs3) and np.array_equal(valid2, valid3) and valid2.all()
    assert _bytes(recs2) != _bytes(recs0)
    assert _pose_bytes(poses2) == _pose_bytes(fresh.detector.last_tag_poses(tpd, raw=True))
    fresh.detector.close()
    det.close()


def test_tag_poses_with_a_camera_work_on_the_normalised_points(scene):
    """ck_estimate_tag_poses with an EUCM set = the same call, no camera set, on the detections' corners replaced by the host twin's
    normalised points under the identity pinhole (fx = fy = 1, cx = cy = 0: its first fixed-point step returns the point itself):
    R, t and the errors byte for byte (H is the pixel homography and differs).  A tag with a corner behind the image plane is invalid."""
    from chalkydri_amd import camera
    from chalkydri_amd.detector import AprilTagDetector, tag_pose_params
    det = AprilTagDetector(W, H)
    dets = det.detect(scene["frame"])
    assert len(dets) >= 2
    cam = camera.make_camera("EUCM", F, F * 1.01, W / 2.0 + 3, H / 2.0 - 2, 0.6, 1.1)
    raw = (A.Detection * len(dets))()
    norm = (A.Detection * len(dets))()
    for i, d in enumerate(dets):
        xy, ok = camera.normalize_host(cam, d.corners())
        assert ok.all()
        for r, pts in ((raw[i], d.corners()), (norm[i], xy)):
            r.id, r.family = d.id(), d.family()
            for k in range(4):
                r.p[k][0], r.p[k][1] = pts[k]
    want = det.estimate_tag_poses(norm, tag_pose_params(1.0, 1.0, 0.0, 0.0), raw=True)
    det.set_camera(cam)
    got = det.estimate_tag_poses(raw, tag_pose_params(123.0, 77.0, 1.0, 2.0, distortion=(1.0,) * 5), raw=True)
    for g, w_ in zip(got, want):
        assert g.valid and w_.valid
        for f in ("id", "valid", "has_alt", "err", "err_alt"):
            assert getattr(g, f) == getattr(w_, f), f
        for f in ("R", "t", "R_alt", "t_alt"):
            assert bytes(getattr(g, f)) == bytes(getattr(w_, f)), f
    # alpha = 0.8, beta chosen so that kz = 0 (r2 = 1 / (alpha^2 beta)) passes through the centre of the tag farthest from the
    # principal point: its outer corners have no normalised point
    i, r2 = _farthest(dets)
    back = camera.make_camera("EUCM", F, F, W / 2.0, H / 2.0, 0.8, 1.0 / (0.64 * r2))
    okn = camera.normalize_host(back, dets[i].corners())[1]
    assert okn.any() and not okn.all()
    det.set_camera(back)
    p = det.estimate_tag_poses(raw, tag_pose_params(F, F, W / 2.0, H / 2.0), raw=True)
    assert not p[i].valid and p[i].id == dets[i].id() and sum(q.valid for q in p) == len(dets) - 1
    det.close()


@pytest.mark.parametrize("n", [1, 3])
def test_workspace_bearings_are_the_host_twins(scene, n):
    """After ck_process_uploaded with a real EUCM set, ck_last_pose_inputs returns, per frame, the host twin's bearings of the known
    detections' corners, in detection order, byte for byte; a detection with one corner outside the model's valid disc is left out
    whole (lib.rs:324).  Batches of 1 and of 3 frames, the middle one of the three without tags."""
    from chalkydri_amd import camera
    from chalkydri_amd.rigcal import last_pose_inputs
    blank = np.full((H, W), 128, np.uint8)
    other, _ = scenes.render_view(72, W, H, F, scene["layout"], (2.6, -0.2, -0.04), R2C, noise_amp=1)
    frames = scene["frame"][None] if n == 1 else np.stack([scene["frame"], blank, other])
    task = _task(scene, scene["calib"], max_batch=n)
    det = task.detector
    dets = det.detect_batch(frames)
    assert len(dets[0]) >= 2 and (n == 1 or (len(dets[1]) == 0 and len(dets[2]) >= 2))
    known = {t["ID"] for t in scene["layout"]["tags"]}
    # the disc's edge through the centre of frame 0's tag farthest from the principal point (alpha = 1: r2 < 1 / beta)
    _, r2 = _farthest(dets[0])
    for cam, cut in ((camera.make_camera("EUCM", F, F * 1.01, W / 2.0 + 3, H / 2.0 - 2, 0.62, 1.08), False),
                     (camera.make_camera("EUCM", F, F, W / 2.0, H / 2.0, 1.0, 1.0 / r2), True)):
        det.set_camera(cam)
        recs, valid = task.process_batch(frames, [POSE[2]] * n)
        steps, rec = last_pose_inputs(det, n)
        dropped = 0
        for f in range(n):
            want = []
            for d in dets[f]:
                if d.id() not in known:
                    continue
                b, ok = camera.unproject_host(cam, d.corners())
                if ok.all():
                    want.append(b)
                else:
                    dropped += 1
                    assert ok.any() or not cut or f > 0                 # the cut tag itself: some corners in, some out
            want = np.concatenate(want) if want else np.zeros((0, 3))
            assert rec[f].n_tags == len(want) // 4 and steps[f][1].tobytes() == want.tobytes(), (f, cut)
        assert (dropped > 0) == cut
        assert cut or valid[0]
    det.close()


def _warp_to_eucm(frame, lens, f):
    """The pinhole frame (focal f, principal point at the centre) as the EUCM lens of the same size would see it: every pixel -> its
    bearing by the restatement -> the pinhole pixel, bilinear; outside the source the border value."""
    h, w = frame.shape
    ys, xs = np.mgrid[0:h, 0:w]
    b, ok = NC.unproject(lens, np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64))
    assert ok.all() and (b[:, 2] > 0).all()
    u = np.clip(f * b[:, 0] / b[:, 2] + w / 2.0, 0, w - 1.001)
    v = np.clip(f * b[:, 1] / b[:, 2] + h / 2.0, 0, h - 1.001)
    x0, y0 = np.floor(u).astype(int), np.floor(v).astype(int)
    ax, ay = u - x0, v - y0
    src = frame.astype(np.float64)
    out = (src[y0, x0] * (1 - ax) * (1 - ay) + src[y0, x0 + 1] * ax * (1 - ay) + src[y0 + 1, x0] * (1 - ax) * ay + src[y0 + 1, x0 + 1] * ax * ay)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8).reshape(h, w)


def _errors(rec, truth):
    pos = float(np.hypot(rec.pose_x - truth["twr"][0], rec.pose_y - truth["twr"][1]))
    yaw = float(abs((rec.pose_rot - truth["yaw"] + np.pi) % (2 * np.pi) - np.pi))
    return pos, yaw


def test_end_to_end_from_eucm_pixels(scene):
    """The scene rendered with the pinhole renderer and resampled in numpy into the image of an EUCM lens (fx = fy = f, alpha = 0.6,
    beta = 1, the issue's lens).  Required: the pose from (warped frame, EUCM model) is within twice the position and yaw error of
    (original frame, pinhole model) plus 1 mm / 1e-3 rad (the factor two is for the resampling blur), and the pose from (warped frame,
    pinhole model) is strictly worse in position than the one with the EUCM model.  Figures in DESIGN.md §4p."""
    lens = (F, F, W / 2.0, H / 2.0, 0.6, 1.0)
    warped = _warp_to_eucm(scene["frame"], lens, F)
    gyro = [POSE[2]]
    pin = _task(scene, scene["calib"])
    r_orig, v_orig = pin.process_batch(scene["frame"][None], gyro)
    r_wpin, v_wpin = pin.process_batch(warped[None], gyro)
    pin.detector.close()
    euc = _task(scene, {"EUCM": dict(fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, alpha=0.6, beta=1.0, width=W, height=H)})
    assert euc.camera.model == A.CK_CAMERA_EUCM and euc.detector.camera is euc.camera
    r_weuc, v_weuc = euc.process_batch(warped[None], gyro)
    euc.detector.close()
    assert v_orig[0] and v_weuc[0] and r_orig[0].tag_count >= 2 and r_weuc[0].tag_count >= 2
    e_orig, e_weuc = _errors(r_orig[0], scene["truth"]), _errors(r_weuc[0], scene["truth"])
    e_wpin = _errors(r_wpin[0], scene["truth"]) if v_wpin[0] else (float("inf"), float("inf"))
    print("pose errors (m, rad): original+pinhole", e_orig, "warped+EUCM", e_weuc, "warped+pinhole", e_wpin,
          "tags", r_orig[0].tag_count, r_weuc[0].tag_count)
    assert e_weuc[0] <= 2 * e_orig[0] + 1e-3 and e_weuc[1] <= 2 * e_orig[1] + 1e-3
    assert e_wpin[0] > e_weuc[0]


def test_misuse(scene):
    """A camera that ck_camera_check refuses leaves the previous setting in place (the next call returns the same bytes); a null
    handle is refused."""
    from chalkydri_amd import camera
    from chalkydri_amd._lib import ChalkydriError
    task = _task(scene, scene["calib"])
    det = task.detector
    good = camera.make_camera("EUCM", F, F, W / 2.0, H / 2.0, 0.3, 1.2)
    det.set_camera(good)
    recs0, valid0 = task.process_batch(scene["frame"][None], [POSE[2]])
    bad = A.Camera()
    bad.model = 7
    for i, v in enumerate((F, F, W / 2.0, H / 2.0, 0.3, 1.2)):
        bad.k[i] = v
    worse = A.Camera.from_buffer_copy(good)
    worse.k[4] = 1.5
    for b in (bad, worse):
        with pytest.raises(ChalkydriError) as e:
            det.set_camera(b)
        assert e.value.code == A.CK_EINVAL and det.camera is good
        recs1, valid1 = task.process_batch(scene["frame"][None], [POSE[2]])
        assert _bytes(recs1) == _bytes(recs0) and np.array_equal(valid0, valid1)
    det.set_camera(None)                                                      # ... and it was a setting: without it the pinhole's bytes differ
    recs2, _ = task.process_batch(scene["frame"][None], [POSE[2]])
    assert valid0[0] and _bytes(recs2) != _bytes(recs0)
    assert det._L.ck_set_camera(None, C.byref(good)) == A.CK_EINVAL
    det.close()
