"""quad_sigma on the device: the filtered quad image equals the numpy restatement of the contract byte for byte, and every stage
after it equals the oracle run on that image — threshold, segmentation, clusters, quads, detections and
pose records; at quad_decimate 2 refinement and decode keep reading the unfiltered frame, at quad_decimate 1 they read Q.  With
the filter off nothing changes."""
import ctypes as C

import numpy as np
import pytest

import quad_filter_ref as R
import scenes
from chalkydri_amd import _abi as A
from chalkydri_amd import default_config, synth
from chalkydri_amd._lib import ChalkydriError
from chalkydri_amd.detector import AprilTagDetector

pytestmark = pytest.mark.gpu
SIGMAS = [0.5, 0.8, 1.0, 1.6, 3.0, 8.0, -0.8, -1.5]


def _frames(seed, w, h, n=2, noise=3):
    """n different frames: rendered tags where they fit, random bytes on top of a gradient where they do not"""
    if w >= 200 and h >= 150:
        return synth.render_batch(seed, n, w, h, 3, noise_amp=noise)[0]
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w), dtype=np.uint8)


@pytest.mark.parametrize("w,h", [(640, 480), (272, 200), (641, 479), (16, 16), (1280, 800)])
@pytest.mark.parametrize("dec", [1, 2])
def test_quad_image_equals_the_restatement(built, w, h, dec):
    n = 2
    frames = _frames(w + h + dec, w, h, n)
    det = AprilTagDetector(w, h, max_batch=n, quad_decimate=dec)
    for sigma in SIGMAS:
        det.set_quad_sigma(sigma)
        got = det.quad_image(frames)
        for i in range(n):
            want = R.quad_image(frames[i], sigma, dec)
            assert np.array_equal(got[i], want), (sigma, i, int((got[i] != want).sum()))
    det.set_quad_sigma(0.0)
    got = det.quad_image(frames)
    for i in range(n):
        assert np.array_equal(got[i], R.decimate(frames[i], dec) if dec > 1 else frames[i])
    det.close()


@pytest.mark.parametrize("dec", [1, 2])
def test_strided_host_frames_and_staged_frames(built, dec):
    w, h, n, pad = 641, 479, 2, 37
    frames = _frames(5, w, h, n)
    padded = np.full((n, h, w + pad), 0xEE, np.uint8)
    padded[:, :, :w] = frames
    det = AprilTagDetector(w, h, max_batch=n, quad_decimate=dec, quad_sigma=-1.5)
    imgs = (A.ImageU8 * n)()
    for i in range(n):
        imgs[i].buf, imgs[i].width, imgs[i].height, imgs[i].stride = padded[i].ctypes.data, w, h, w + pad
    out = np.empty((n, h // dec, w // dec), np.uint8)
    assert det._L.ck_quad_image_batch(det._h, imgs, n, out.ctypes.data) == 0
    for i in range(n):
        assert np.array_equal(out[i], R.quad_image(frames[i], -1.5, dec))
    assert np.array_equal(det.quad_image(None, n), out)       # imgs == NULL: the staged frames
    det.close()


def _oracle_stages(oracle, frame, q, cfg, dec):
    th = oracle.threshold(q)
    lab, sz = oracle.segment(th)
    cl, pts, _ = oracle.clusters(th, lab, sz)
    # edge refinement reads the unfiltered frame at quad_decimate 2 and Q itself at 1 (the two decisions)
    quads, _ = oracle.fit_quads(frame if dec > 1 else q, cfg, cl, pts, quad_img=q)
    return th, lab, sz, cl, pts, quads


def _decode(oracle, frame, cfg, quads):
    L = oracle.lib()
    fr = np.ascontiguousarray(frame)
    h, w = fr.shape
    qa = (A.Quad * max(len(quads), 1))(*quads)
    dets = (A.Detection * 256)()
    nd = C.c_int(0)
    L.ora_decode_quads(C.c_void_p(fr.ctypes.data), w, h, w, C.byref(cfg), qa, len(quads), dets, 256, C.byref(nd))
    return oracle.dets_to_list(dets, nd.value)


def _same_dets(have, want):
    assert len(have) == len(want), f"{len(have)} vs {len(want)} detections"
    for a, b in zip(have, want):
        assert (a.id(), a.hamming(), a.family()) == (b["id"], b["hamming"], b["family"])
        assert np.float32(a.decision_margin()) == np.float32(b["margin"])
        assert np.array_equal(a.center(), b["c"]) and np.array_equal(a.corners(), b["p"])


def _quads_np(quads):
    arr = np.zeros((len(quads), 11))
    for i, q in enumerate(quads):
        arr[i, :8] = [q.p[k][j] for k in range(4) for j in range(2)]
        arr[i, 8:] = [q.reversed_border, q.rep0, q.rep1]
    if len(arr):
        arr = arr[np.lexsort((arr[:, 10], arr[:, 9]))]
    return arr


def _cluster_dict(cl, pts, lo=24, hi=1 << 30):
    out = {}
    for rep0, rep1, start, count in cl:
        if count < lo or count > hi:
            continue
        p = pts[start:start + count]
        arr = np.stack([p["x"].astype(np.int64), p["y"].astype(np.int64), p["gx"].astype(np.int64), p["gy"].astype(np.int64)], 1)
        out[(int(rep0), int(rep1))] = arr[np.lexsort((arr[:, 3], arr[:, 2], arr[:, 1], arr[:, 0]))]
    return out


@pytest.mark.parametrize("dec,sigma", [(1, 0.8), (1, -0.8), (2, 0.8), (2, -1.5), (1, 3.0)])
def test_stages_equal_the_oracle_on_the_quad_image(oracle, dec, sigma):
    w, h, n = 640, 480, 2
    frames = _frames(40 + dec, w, h, n, noise=4)
    det = AprilTagDetector(w, h, max_batch=n, quad_decimate=dec, quad_sigma=sigma)
    cfg = default_config(w, h, quad_decimate=dec)
    th = det.threshold(frames)
    labels, sizes = det.segment(frames)
    cls = det.clusters(frames)
    qs = det.quads(frames)
    dets = det.detect_batch(frames)
    qw, qh = w // dec, h // dec
    maxpts = 3 * (2 * qw + 2 * qh)
    for i in range(n):
        q = R.quad_image(frames[i], sigma, dec)
        oth, olab, osz, ocl, opts, oq = _oracle_stages(oracle, frames[i], q, cfg, dec)
        assert np.array_equal(th[i], oth)
        assert np.array_equal(labels[i], olab) and np.array_equal(sizes[i], osz)
        want, have = _cluster_dict(ocl, opts, 24, maxpts), _cluster_dict(*cls[i])
        assert set(want) == set(have)
        for k in want:
            assert np.array_equal(want[k], have[k])
        assert np.array_equal(_quads_np(oq), _quads_np(qs[i]))
        # refinement and decode: Q at quad_decimate 1 (through ora_detect on Q), the frame itself at 2
        wd = oracle.detect(q, cfg)[0] if dec == 1 else _decode(oracle, frames[i], cfg, oq)
        assert len(wd) >= 1
        _same_dets(dets[i], wd)
    det.close()


def _scene(n, w=640, h=480, noise=3, seed=700):
    f = 600.0
    layout = scenes.wall_layout(6, cols=3)
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
    calib = scenes.pinhole_calib(f, w / 2.0, h / 2.0)
    rng = np.random.default_rng(seed)
    frames, gyros = [], []
    for i in range(n):
        pose = (rng.uniform(1.8, 2.4), rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1))
        frames.append(scenes.render_view(seed + i, w, h, f, layout, pose, r2c, noise_amp=noise)[0])
        gyros.append(pose[2])
    return np.stack(frames), gyros, layout, calib, r2c


def test_process_at_full_resolution_equals_the_oracle_on_the_quad_image(oracle):
    """At quad_decimate 1 every stage reads Q: the records with the filter are the records of an unfiltered handle given Q, byte for
    byte, and those equal ora_process_frame(Q) to the pose tests' tolerance (tests/test_gpu_pose.py: the solver's last bits)."""
    from chalkydri_amd.apriltags import AprilTags
    n, w, h, sigma = 3, 640, 480, 0.8
    frames, gyros, layout, calib, r2c = _scene(n)
    task = AprilTags(w, h, layout, calib, r2c, cam_id=3, max_batch=n, quad_sigma=sigma)
    recs, valid = task.process_batch(frames, gyros)
    dets = task.detector.detect_batch(frames, cap=32)
    qs = np.stack([R.quad_image(frames[i], sigma) for i in range(n)])
    plain = AprilTags(w, h, layout, calib, r2c, cam_id=3, max_batch=n)
    precs, pvalid = plain.process_batch(qs, gyros)
    pdets = plain.detector.detect_batch(qs, cap=32)
    assert valid.all() and np.array_equal(valid, pvalid)
    assert [bytes(r) for r in recs] == [bytes(r) for r in precs]
    assert [[(d.id(), d.corners().tobytes()) for d in fr] for fr in dets] == [[(d.id(), d.corners().tobytes()) for d in fr] for fr in pdets]
    cfg = default_config(w, h)
    for i in range(n):
        _same_dets(dets[i], oracle.detect(qs[i], cfg)[0])
        out, v = A.VisionMeasurement(), C.c_int(0)
        oracle.lib().ora_process_frame(C.c_void_p(qs[i].ctypes.data), w, h, w, C.byref(cfg), C.byref(task._pp), C.c_double(float(gyros[i])), 1,
                                       C.byref(out), C.byref(v))
        r = recs[i]
        assert bool(v.value) and (r.camera_id, r.tag_count) == (out.camera_id, out.tag_count)
        assert abs(r.pose_x - out.pose_x) < 1e-6 and abs(r.pose_y - out.pose_y) < 1e-6 and abs(r.pose_rot - out.pose_rot) < 1e-7


@pytest.mark.parametrize("dec", [1, 2])
def test_device_frames_and_ingest_ring_equal_host_frames(built, dec):
    import torch
    from chalkydri_amd.detector import IngestRing
    n, w, h, pad = 3, 640, 480, 16
    frames, *_ = _scene(n, seed=800 + dec)
    det = AprilTagDetector(w, h, max_batch=n, quad_decimate=dec, quad_sigma=-0.8)
    want, wst = det.detect_batch(frames, cap=32, return_status=True)
    key = lambda ds: [[(d.id(), d.corners().tobytes(), d.center().tobytes()) for d in fr] for fr in ds]
    assert sum(len(d) for d in want) >= n
    padded = np.zeros((n, h, w + pad), np.uint8)
    padded[:, :, :w] = frames
    dev = torch.from_numpy(padded).cuda()
    got, gst = det.detect_device(dev.data_ptr(), n, w + pad, (w + pad) * h, cap=32)
    assert key(got) == key(want) and list(gst) == list(wst)
    packed = torch.from_numpy(np.ascontiguousarray(frames[:, :, 1:])).cuda()   # rows of 639 bytes: restaged by the library
    det2 = AprilTagDetector(w - 1, h, max_batch=n, quad_decimate=dec, quad_sigma=-0.8)
    want2 = det2.detect_batch(np.ascontiguousarray(frames[:, :, 1:]), cap=32)
    got2, _ = det2.detect_device(packed.data_ptr(), n, w - 1, (w - 1) * h, cap=32)
    assert key(got2) == key(want2)
    ring = IngestRing(det, n_slots=1)
    ring.slot_view(0)[:, :, :w] = frames
    ring.submit(0, n)
    got3, st3 = ring.detect(0, n, cap=32)
    assert key(got3) == key(want) and list(st3) == list(wst)
    ring.close()
    det.close(); det2.close()


@pytest.mark.parametrize("dec", [1, 2])
def test_filter_off_changes_nothing(built, dec):
    from chalkydri_amd.apriltags import AprilTags
    n = 3
    frames, gyros, layout, calib, r2c = _scene(n, seed=950)

    def run(setting):
        task = AprilTags(640, 480, layout, calib, r2c, cam_id=1, max_batch=n, quad_decimate=dec)
        for s in setting:
            task.detector.set_quad_sigma(s)
        recs, valid = task.process_batch(frames, gyros)
        dets, st = task.detector.detect_batch(frames, cap=32, return_status=True)
        out = ([bytes(r) for r in recs], list(valid), list(st), [[(d.id(), d.corners().tobytes()) for d in fr] for fr in dets])
        task.detector.close()
        return out

    base = run([])
    assert sum(base[1]) == n
    for setting in ([0.0], [0.3], [-0.49], [0.8, 0.0]):
        assert run(setting) == base, setting


def test_blur_still_finds_every_tag_in_heavy_noise(built):
    w, h, n = 640, 480, 3
    frames, truths = synth.render_batch(77, n, w, h, 4, noise_amp=24)
    det = AprilTagDetector(w, h, max_batch=n, quad_sigma=0.8)
    dets = det.detect_batch(frames, cap=64)
    for i in range(n):
        assert {t["id"] for t in truths[i]} <= {d.id() for d in dets[i]}, i
    det.close()


def test_misuse_is_refused(built):
    det = AprilTagDetector(64, 64, max_batch=2)
    L = det._L
    frames = _frames(1, 64, 64, 3)
    assert L.ck_set_quad_sigma(None, 1.0) == A.CK_EINVAL
    assert L.ck_set_quad_sigma(det._h, float("nan")) == A.CK_EINVAL
    assert L.ck_set_quad_sigma(det._h, 8.5) == A.CK_EUNSUPPORTED
    assert L.ck_set_quad_sigma(det._h, -9.0) == A.CK_EUNSUPPORTED
    assert L.ck_quad_image_batch(None, None, 1, None) == A.CK_EINVAL
    with pytest.raises(ChalkydriError) as e:
        det.quad_image(frames)                                    # 3 frames on a handle made for 2
    assert e.value.code == A.CK_ECAPACITY
    from chalkydri_amd.detector import _images
    arr, keep = _images(frames[:2])
    assert L.ck_quad_image_batch(det._h, arr, 2, None) == A.CK_EINVAL
    det.set_quad_sigma(1.0)
    with pytest.raises(ChalkydriError):
        det.set_quad_sigma(float("inf"))
    got = det.quad_image(frames[:2])                              # the refused values left the handle as it was
    assert np.array_equal(got[0], R.quad_image(frames[0], 1.0)) and np.array_equal(got[1], R.quad_image(frames[1], 1.0))
    det.close()
