"""Sub-pixel corners on the MI355X (k_subpix, k_subpix_dets, k_board): ck_corner_subpix returns the host twin's bytes
for every window, point count and pointer kind; the detector setting replaces a call's corners by exactly that refinement and
everything downstream inherits them; ck_board_corners_last returns ck_board_corners_host's bytes; the Calibrator keeps more of an
AprilGrid with recovery on."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_board_render as BR  # noqa: E402
import np_tag_render as NR  # noqa: E402
import scenes  # noqa: E402
import subpix_scenes as SC  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

SW, SH = 160, 120
CAP = 64
FLAT = 24   # the small frames' constant block: [0, FLAT)^2


@pytest.fixture(scope="module")
def small(built):
    """three 160 x 120 frames with one 60-pixel tag each and a constant block of 24 x 24 pixels in a corner, and a detector that has
    them staged"""
    from chalkydri_amd import _lib
    from chalkydri_amd.detector import AprilTagDetector
    fam = _lib.family("tag36h11")
    frames, corners = [], []
    for i in range(3):
        tag = {"fam": fam, "code": int(NR.family_gen.tables(fam)[6][7 + i]), "corners": NR.pose(78 + 3 * i, 61 - 2 * i, 60, 11.0 * i - 8, (0.02, -0.03))}
        img, truth = NR.render(SW, SH, [tag], seed=40 + i, noise=2.0)
        img[:FLAT, :FLAT] = 90 + i
        frames.append(img)
        corners.append(truth[0]["corners"])
    det = AprilTagDetector(SW, SH, max_batch=3)
    frames = np.stack(frames)
    det.upload(frames)
    yield det, frames, np.array(corners)
    det.close()


@pytest.fixture(scope="module")
def big(built):
    """the 643 x 481 board views (a width that is no multiple of 64) and a detector of that size for three frames"""
    from chalkydri_amd.detector import AprilTagDetector
    det = AprilTagDetector(SC.W, SC.H, max_batch=3)
    blank = np.clip(np.rint(128 + np.random.default_rng(5).normal(0, 2.0, (SC.H, SC.W))), 0, 255).astype(np.uint8)
    frames = np.stack([SC.board_frame(2, 0.8)[0], SC.board_frame(1, 0.8, True)[0], blank])
    yield det, frames
    det.close()


def _points(rng, n, w, h, corners, n_frames, flat=0):
    """n points and their frames: tag corners with up to a pixel of jitter, spots anywhere and in the constant block, points on and
    near the frame edge, points on integer coordinates; every frame, in shuffled order"""
    fr = rng.integers(0, n_frames, n).astype(np.int32)
    kind = rng.integers(0, 4, n)
    xy = np.empty((n, 2))
    for i in range(n):
        if kind[i] == 0 or n < 4:
            xy[i] = corners[fr[i]][rng.integers(0, len(corners[fr[i]]))] + rng.uniform(-1, 1, 2)
        elif kind[i] == 1:
            xy[i] = rng.uniform([0, 0], [flat, flat] if flat and i % 2 else [w, h])
        elif kind[i] == 2:
            xy[i] = [(0.0, w, rng.uniform(0, 3), w - rng.uniform(0, 3))[rng.integers(0, 4)], (0.0, h, rng.uniform(0, 3), h - rng.uniform(0, 3))[rng.integers(0, 4)]]
        else:
            xy[i] = np.rint(corners[fr[i]][rng.integers(0, len(corners[fr[i]]))] + rng.uniform(-2, 2, 2))
    return fr, np.clip(xy, 0, [w, h])


def _device_call(det, pp, fr, xy):
    import torch
    n = len(xy)
    d_fr, d_xy = torch.from_numpy(fr).cuda(), torch.from_numpy(xy).cuda()
    d_out, d_info = torch.zeros((n, 2), dtype=torch.float64, device="cuda"), torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = det._L.ck_corner_subpix(det._h, C.byref(pp), C.c_void_p(d_fr.data_ptr()), C.c_void_p(d_xy.data_ptr()), n, C.c_void_p(d_out.data_ptr()),
                                 C.c_void_p(d_info.data_ptr()))
    assert rc == 0
    return d_out.cpu().numpy(), d_info.cpu().numpy().tobytes()


@pytest.mark.parametrize("w", [2, 5, 7])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_device_returns_the_host_bytes(small, big, n, w):
    from chalkydri_amd import subpix
    pp = subpix.subpix_params(half_win=w)
    rng = np.random.default_rng(1000 * w + n)
    det, frames, corners = small
    bdet, bframes = big
    bdet.upload(bframes[:1])
    bcorners = [SC.board_frame(2, 0.8)[1]["uv"].reshape(-1, 2)]
    for d, fs, cs, flat in ((det, frames, corners, FLAT), (bdet, bframes[:1], bcorners, 0)):
        fr, xy = _points(rng, n, fs.shape[2], fs.shape[1], cs, len(fs), flat)
        want, winfo = subpix.corner_subpix_host(fs, fr, xy, pp, return_info=True)
        got, ginfo = d.corner_subpix(fr, xy, pp, return_info=True)
        assert got.tobytes() == want.tobytes() and ginfo.tobytes() == winfo.tobytes()
        dgot, dinfo = _device_call(d, pp, fr, xy)
        assert dgot.tobytes() == want.tobytes() and dinfo == winfo.tobytes()
        if n >= 63:
            assert (winfo["status"] == A.CK_SUBPIX_CONVERGED).sum() >= n // 8
        if n == 1000:  # every status is among them (FLAT: the constant block of the small frames)
            assert set(winfo["status"]) == ({0, 1, 2, 3} if flat else {0, 1, 3})


def test_device_refusals(small):
    from chalkydri_amd import subpix
    from chalkydri_amd._lib import ChalkydriError
    det, frames, corners = small
    for args in (dict(frame=3, xy=[[80.0, 60.0]]), dict(frame=-1, xy=[[80.0, 60.0]]), dict(frame=0, xy=[[np.nan, 1.0]]), dict(frame=0, xy=[[SW + 0.5, 1.0]]),
                 dict(frame=0, xy=[[1.0, -0.5]]), dict(frame=0, xy=[[80.0, 60.0]], params=subpix.subpix_params(half_win=8))):
        with pytest.raises(ChalkydriError) as e:
            det.corner_subpix(**args)
        assert e.value.code == A.CK_EINVAL
    assert det.corner_subpix(0, np.zeros((0, 2))).shape == (0, 2)
    with pytest.raises(ChalkydriError):
        det.set_corner_subpix(max_iters=0)
    assert det.corner_subpix_params is None


def _detect_raw(det, n, frames=None, device=None):
    """the ck_detection_t records of a detect call, as bytes per frame"""
    dets, counts, status = (A.Detection * (n * CAP))(), (C.c_int32 * n)(), (C.c_uint32 * n)()
    C.memset(dets, 0, C.sizeof(dets))
    if device is not None:
        ptr, stride, pitch = device
        assert det._L.ck_detect_batch_device(det._h, C.c_void_p(ptr), n, stride, pitch, dets, CAP, counts, status) == 0
    elif frames is not None:
        from chalkydri_amd.detector import _images
        arr, keep = _images(frames)
        assert det._L.ck_detect_batch(det._h, arr, n, dets, CAP, counts, status) == 0
    else:
        assert det._L.ck_detect_uploaded(det._h, n, dets, CAP, counts, status) == 0
    return [[A.Detection.from_buffer_copy(dets[i * CAP + k]) for k in range(counts[i])] for i in range(n)]


def _bytes(per_frame):
    return b"".join(bytes(d) for fr in per_frame for d in fr)


@pytest.mark.parametrize("decimate", [1, 2])
def test_setting_on_is_the_refinement_of_the_call_with_it_off(built, decimate):
    """ck_detect_uploaded with the setting on = the same call with it off, `p` replaced by ck_corner_subpix of those corners on the
    staged frames, bit for bit, and `c` by the image of the tag centre under the new corners' homography; the same through
    ck_detect_batch_device with a stride above the width; setting NULL again restores the first result byte for byte."""
    import torch
    from chalkydri_amd import subpix
    from chalkydri_amd.detector import AprilTagDetector
    frames = np.stack([SC.board_frame(2, 0.0)[0], SC.board_frame(0, 0.8)[0], SC.board_frame(3, 0.8)[0]])
    det = AprilTagDetector(SC.W, SC.H, max_batch=3, quad_decimate=decimate)
    det.upload(frames)
    off = _detect_raw(det, 3)
    assert sum(len(f) for f in off) >= 8
    for w in (5, 3):
        det.set_corner_subpix(half_win=w)
        on = _detect_raw(det, 3)
        pp = subpix.subpix_params(half_win=w)
        moved = 0
        for f in range(3):
            assert len(on[f]) == len(off[f])
            for a, b in zip(off[f], on[f]):
                assert (a.id, a.hamming, a.family, a.decision_margin) == (b.id, b.hamming, b.family, b.decision_margin)
                p = np.array([[a.p[k][0], a.p[k][1]] for k in range(4)])
                want = det.corner_subpix(f, p, pp)
                assert bytes(b.p) == want.tobytes()
                if want.tobytes() == p.tobytes():
                    assert bytes(b) == bytes(a)
                    continue
                moved += 1
                Hm = NR.homography(want[[3, 2, 1, 0]])       # (-1,-1), (1,-1), (1,1), (-1,1) <- corners 3, 2, 1, 0
                assert np.abs(np.array(NR.project(Hm, 0.0, 0.0)) - [b.c[0], b.c[1]]).max() < 1e-9
        assert moved >= 8
        pad = 29
        padded = np.full((3, SC.H, SC.W + pad), 0x5A, np.uint8)
        padded[:, :, :SC.W] = frames
        d = torch.from_numpy(padded).cuda()
        torch.cuda.synchronize()
        assert _bytes(_detect_raw(det, 3, device=(d.data_ptr(), SC.W + pad, (SC.W + pad) * SC.H))) == _bytes(on)
        assert _bytes(_detect_raw(det, 3, frames=frames)) == _bytes(on)
    det.set_corner_subpix(on=False)
    assert _bytes(_detect_raw(det, 3)) == _bytes(off)
    det.close()


def test_pose_inputs_carry_the_refined_corners(built):
    """After ck_process_uploaded with the setting on, ck_last_pose_inputs holds ck_camera_unproject's bearings of the refined corners
    (= the detections of a detect call with the setting on) of the known tags, byte for byte; the tag poses inherit them too."""
    from chalkydri_amd import camera
    from chalkydri_amd.apriltags import AprilTags
    from chalkydri_amd.detector import tag_pose_params
    from chalkydri_amd.rigcal import last_pose_inputs
    w, h, f = 640, 480, 576.0
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
    layout = scenes.wall_layout(6, cols=3)
    f0, _ = scenes.render_view(71, w, h, f, layout, (2.2, 0.1, 0.05), r2c, noise_amp=1)
    f1, _ = scenes.render_view(72, w, h, f, layout, (2.6, -0.2, -0.04), r2c, noise_amp=1)
    frames = np.stack([f0, f1])
    calib = scenes.pinhole_calib(f, w / 2.0, h / 2.0)
    plain = AprilTags(w, h, layout, calib, r2c, cam_id=3, max_batch=2)
    task = AprilTags(w, h, layout, calib, r2c, cam_id=3, max_batch=2, corner_subpix=dict(half_win=4))
    recs0, valid0 = plain.process_batch(frames, [0.05, -0.04])
    recs, valid = task.process_batch(frames, [0.05, -0.04])
    assert valid.all() and valid0.all() and bytes(recs[0]) != bytes(recs0[0])
    steps, rec = last_pose_inputs(task.detector, 2)
    tpp = tag_pose_params(f, f, w / 2.0, h / 2.0)
    poses = task.detector.last_tag_poses(tpp, raw=True)
    dets = task.detector.detect_batch(frames)
    assert [bytes(p) for fr in poses for p in fr] == [bytes(p) for fr in task.detector.last_tag_poses(tpp, raw=True) for p in fr]
    base = plain.detector.detect_batch(frames)
    known = {t["ID"] for t in layout["tags"]}
    for i in range(2):
        assert len(dets[i]) == len(base[i]) >= 2
        want = [camera.unproject(task.camera, d.corners())[0] for d in dets[i] if d.id() in known]
        assert rec[i].n_tags == len(want) and steps[i][1].tobytes() == np.concatenate(want).tobytes()
        assert any(d.corners().tobytes() != b.corners().tobytes() for d, b in zip(dets[i], base[i]))
        assert max(np.abs(d.corners() - b.corners()).max() for d, b in zip(dets[i], base[i])) <= 4.0   # (half_win: the rejection bound)
    task.detector.close()
    plain.detector.close()


def test_board_recovery_returns_the_host_bytes(big):
    """ck_board_corners_last = ck_board_corners_host on the call's own detections: two board views (one with a painted patch) and a
    frame without any tag in one call; a 1 x 1 board; the validity rule."""
    from chalkydri_amd import subpix
    from chalkydri_amd._lib import ChalkydriError
    from chalkydri_amd.calibration import Board
    det, frames = big
    det.upload(frames)
    dets = _detect_raw(det, 3)
    assert len(dets[0]) >= 3 and len(dets[1]) >= 2 and len(dets[2]) == 0
    board = SC.board()
    uv, state = det.board_corners(board)
    wuv, wstate = subpix.board_corners_host(board, frames, dets)
    assert uv.shape == (3, 16, 4, 2) and uv.tobytes() == wuv.tobytes() and state.tobytes() == wstate.tobytes()
    truth, hidden = SC.board_frame(2, 0.8)[1], SC.board_frame(1, 0.8, True)[1]
    assert (state[0] > 0).all() and 1 <= (state[0] == 1).sum() <= len({d.id for d in dets[0] if d.hamming == 0 and d.id < 16})
    assert np.abs(uv[0] - truth["uv"]).max() < 0.6
    assert (state[1][hidden["clear"]] > 0).all() and not state[1][hidden["hidden"]].any() and not state[2].any() and not uv[2].any()
    # other parameters, device pointers
    import torch
    pp, bp = subpix.subpix_params(half_win=4), subpix.board_params(max_shift=1.5)
    wuv, wstate = subpix.board_corners_host(board, frames, dets, pp, bp)
    d_uv, d_st = torch.zeros(3 * 16 * 8, dtype=torch.float64, device="cuda"), torch.zeros(3 * 16, dtype=torch.uint8, device="cuda")
    d_nt = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bd = subpix.board_desc(board)
    assert det._L.ck_board_corners_last(det._h, C.byref(bd), C.byref(pp), C.byref(bp), C.c_void_p(d_uv.data_ptr()), C.c_void_p(d_st.data_ptr()),
                                        C.c_void_p(d_nt.data_ptr())) == 0
    assert d_uv.cpu().numpy().tobytes() == wuv.tobytes() and d_st.cpu().numpy().tobytes() == wstate.tobytes()
    assert d_nt.cpu().numpy().tolist() == [int((s > 0).sum()) for s in wstate]
    # a board of one tag: the seed alone, or nothing
    one = Board(1, 1, board.tag_size, board.tag_spacing, first_id=int(dets[0][0].id))
    uv1, st1 = det.board_corners(one)
    w1, ws1 = subpix.board_corners_host(one, frames, dets)
    assert uv1.tobytes() == w1.tobytes() and st1.tobytes() == ws1.tobytes() and st1[0, 0] == 1 and not st1[2].any()
    # refusals: a family the handle does not have, too many tags, a workspace another call rewrote
    for bad in (dict(family=1), dict(board=Board(9, 8))):
        with pytest.raises(ChalkydriError) as e:
            det.board_corners(bad.get("board", board), family=bad.get("family", 0))
        assert e.value.code == A.CK_EINVAL
    det.quads(n=1)
    with pytest.raises(ChalkydriError) as e:
        det.board_corners(board)
    assert e.value.code == A.CK_EINVAL


def test_calibrator_keeps_more_of_the_board_with_recovery(built):
    """Eight noise-free views of the AprilGrid (pinhole, f = 0.9 w, principal point at the centre): Calibrator(recover=True) keeps more
    points per frame than the plain path, and its intrinsics are no further from the truth.  Measured: 6 frames x 64 points, 0.63 px
    from the truth (rms 0.085 px) against 5 frames of 8 to 24 points, 8.1 px (rms 0.296 px)."""
    from chalkydri_amd import _lib
    from chalkydri_amd import calibration as K
    from chalkydri_amd.detector import AprilTagDetector
    fam = _lib.family("tag36h11")
    frames = np.stack([BR.render(fam, seed=s, blur=0.0, noise=0.0)[0] for s in range(8)])
    det = AprilTagDetector(SC.W, SC.H, max_batch=8)
    truth = np.array([0.9 * SC.W, 0.9 * SC.W, SC.W / 2.0, SC.H / 2.0])
    got = {}
    for recover in (False, True):
        cal = K.Calibrator(det, SC.board(), min_corners=8, recover=recover)
        kept = cal.process(frames)
        pts = [len(u) for _, u in cal.observations()]
        res = cal.calibrate(fixed_mask=K.FIX_DISTORTION)
        err = np.inf if res is None else float(np.abs(np.array([res[0]["OpenCVModel5"][k] for k in ("fx", "fy", "cx", "cy")]) - truth).max())
        got[recover] = (kept, pts, err, None if res is None else res[1]["rms"])
        print("recover", recover, "frames", kept, "points per frame", pts, "max |fx fy cx cy - truth|", err, "rms", got[recover][3])
    # (without noise the squares merge with the tags' borders most cleanly: some views decode no tag at all, and nothing starts there)
    assert got[True][0] >= 5 and all(p == 64 for p in got[True][1])
    assert got[True][0] >= got[False][0] and np.mean(got[True][1]) > np.mean(got[False][1] or [0])
    assert got[True][2] <= got[False][2]
    det.close()
