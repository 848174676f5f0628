"""Raw camera formats and orientation on the device: the staged luma is byte-equal to the numpy restatement
(tests/raw_format_ref.py) for every format family, orientation, size, stride and base offset, and everything behind the staged
frames — detections, pose records, the ingest ring, the quad-image settings — returns what it returns behind ck_upload_frames.
Nothing here has a tolerance: nothing here is floating point before the detector, and the detector is deterministic."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raw_format_ref as R  # noqa: E402
import scenes  # noqa: E402
import stress_raw_format as S  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

STRIDE_EXTRA = (0, 5, 24)
OFFSETS = (0, 1, 7)


def det_key(d):
    return (d.id(), d.hamming(), d.family(), np.float32(d.decision_margin()).tobytes(), d.center().tobytes(), d.corners().tobytes())


def keys(dets):
    return [[det_key(d) for d in frame] for frame in dets]


def offset_view(packed, off):
    """The same bytes `off` bytes into a fresh buffer: a source whose base pointer is not aligned."""
    raw = np.full(packed.size + off + 32, 0x3C, np.uint8)
    base = (-raw.ctypes.data) % 16 + off          # (raw + base) % 16 == off
    raw[base:base + packed.size] = packed.reshape(-1)
    v = raw[base:base + packed.size].reshape(packed.shape)
    assert v.ctypes.data % 16 == off % 16
    return v


@pytest.mark.parametrize("W,H", [(16, 16), (272, 200), (641, 479), (640, 480), (1280, 800)])
def test_luma_equals_restatement(built, W, H):
    """ck_raw_luma_batch for every family x orientation at one oriented size; the nine stride x base-offset variants of a source
    are the nine frames of one call.  Random content; pad bytes, chroma and alpha are unlike the luma."""
    from chalkydri_amd.detector import AprilTagDetector
    det = AprilTagDetector(W, H, max_batch=len(STRIDE_EXTRA) * len(OFFSETS))
    rng = np.random.default_rng(W * 10000 + H)
    for fourcc in R.FAMILIES:
        for o in R.ORIENTATIONS:
            sw, sh = R.source_size(W, H, o)
            views, want = [], []
            for extra in STRIDE_EXTRA:
                for off in OFFSETS:
                    stride = R.min_stride(fourcc, sw) + extra
                    img = rng.integers(0, 256, (sh, sw, 3) if R.is_colour(fourcc) else (sh, sw), dtype=np.uint8)
                    v = offset_view(R.pack(img, fourcc, stride, pad_byte=0xA7 ^ extra, seed=int(rng.integers(1 << 30))), off)
                    views.append(v)
                    want.append(R.expected(v, fourcc, sw, sh, stride, o))
            got = det.raw_luma(views, fourcc, o)
            for i, w_ in enumerate(want):
                bad = int((got[i] != w_).sum())
                assert bad == 0, (fourcc, o, W, H, STRIDE_EXTRA[i // 3], OFFSETS[i % 3], bad)
    # the loop form of the restatement on one small case per family, so the vectorised form is not its own judge here
    if W == 16:
        for fourcc in R.FAMILIES:
            img = rng.integers(0, 256, (16, 16, 3) if R.is_colour(fourcc) else (16, 16), dtype=np.uint8)
            buf = R.pack(img, fourcc, R.min_stride(fourcc, 16) + 5)
            want = R.orient(R.luma(buf, fourcc, 16, 16, buf.shape[1]), "clockwise")
            assert np.array_equal(det.raw_luma([buf], fourcc, "clockwise")[0], want), fourcc
    det.close()


def test_every_fourcc_name_of_a_family_is_the_same_bytes(built):
    from chalkydri_amd.detector import AprilTagDetector
    W, H = 48, 32
    det = AprilTagDetector(W, H, max_batch=1)
    rng = np.random.default_rng(5)
    for fourcc in R.FOURCCS:
        img = rng.integers(0, 256, (H, W, 3) if R.is_colour(fourcc) else (H, W), dtype=np.uint8)
        buf = R.pack(img, fourcc)
        assert np.array_equal(det.raw_luma([buf], fourcc)[0], R.expected(buf, fourcc, W, H, buf.shape[1], "none")), fourcc
    det.close()


def wall_frames(n, w=640, h=480, f=600.0, seed=8):
    layout = scenes.wall_layout(6, cols=3)
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
    rng = np.random.default_rng(seed)
    frames, gyros = [], []
    for i in range(n):
        pose = (rng.uniform(1.8, 2.4), rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1))
        fr, _ = scenes.render_view(500 + i, w, h, f, layout, pose, r2c, noise_amp=2)
        frames.append(fr); gyros.append(pose[2])
    return np.stack(frames), gyros, layout, r2c, scenes.pinhole_calib(f, w / 2.0, h / 2.0)


def test_detections_equal_the_plain_path(built):
    """upload_raw(pack(frame)) + detect_uploaded returns the bytes of detect_batch(frame): exact by construction for the Y
    formats; for colour sources the comparison frame is the restatement's luma; with an orientation it is the turned frame on a
    handle of the turned geometry.  Every tag of the scene is found under its id."""
    from chalkydri_amd.detector import AprilTagDetector
    n = 2
    frames, _, _, _, _ = wall_frames(n)
    h, w = frames.shape[1:]
    ids = [1, 2, 3, 4, 5, 6]
    handles = {}
    for o in R.ORIENTATIONS:
        W, H = (h, w) if o in ("clockwise", "counterclockwise") else (w, h)     # the source is always the camera's w x h
        if (W, H) not in handles:
            handles[(W, H)] = AprilTagDetector(W, H, max_batch=n)
        det = handles[(W, H)]
        turned = np.stack([R.orient_vec(f, o) for f in frames])
        want = keys(det.detect_batch(turned))
        assert all(sorted(k[0] for k in fr) == ids for fr in want), o
        for fourcc in ("YUYV", "UYVY", "NV12", "GREY"):
            src = [R.pack(f, fourcc, R.min_stride(fourcc, w) + 8, seed=3) for f in frames]
            assert det.upload_raw(src, fourcc, o) == n
            assert keys(det.detect_batch(None, n=n)) == want, (fourcc, o)
        for fourcc in ("RGB3", "BGR3", "RGBA", "BGRA"):
            rgb = [R.grey_to_rgb(f, seed=i) for i, f in enumerate(frames)]
            src = [R.pack(c, fourcc, seed=4) for c in rgb]
            lum = np.stack([R.orient_vec(R.L(c[..., 0], c[..., 1], c[..., 2]), o) for c in rgb])
            want_rgb = keys(det.detect_batch(lum))
            assert all(sorted(k[0] for k in fr) == ids for fr in want_rgb), (fourcc, o)
            det.upload_raw(src, fourcc, o)
            assert keys(det.detect_batch(None, n=n)) == want_rgb, (fourcc, o)
    for d in handles.values():
        d.close()


def test_process_records_equal_the_plain_path(built):
    from chalkydri_amd.apriltags import AprilTags
    n = 3
    frames, gyros, layout, r2c, calib = wall_frames(n)
    h, w = frames.shape[1:]
    plain = AprilTags(w, h, layout, calib, r2c, cam_id=2, max_batch=n)
    want, valid = plain.process_batch(frames, gyros)
    assert valid.all()
    for fourcc in ("YUYV", "UYVY", "GREY"):
        task = AprilTags(w, h, layout, calib, r2c, cam_id=2, max_batch=n, fourcc=fourcc)
        out, v = task.process_raw_batch([R.pack(f, fourcc, seed=9) for f in frames], gyros)
        assert np.array_equal(v, valid) and [bytes(r) for r in out] == [bytes(r) for r in want], fourcc
        task.detector.close()
    # a camera mounted upside-down: its frames are the scene turned by 180 degrees, the task turns them back
    task = AprilTags(w, h, layout, calib, r2c, cam_id=2, max_batch=n, fourcc="YUYV", orientation="rotate-180")
    out, v = task.process_raw_batch([R.pack(R.source_of(f, "rotate-180"), "YUYV", seed=9) for f in frames], gyros)
    assert np.array_equal(v, valid) and [bytes(r) for r in out] == [bytes(r) for r in want]
    task.detector.close()
    # RGB: against the plain path on the restatement's luma
    rgb = [R.grey_to_rgb(f, seed=i) for i, f in enumerate(frames)]
    lum = np.stack([R.L(c[..., 0], c[..., 1], c[..., 2]) for c in rgb])
    want_rgb, valid_rgb = plain.process_batch(lum, gyros)
    want_rgb = [bytes(r) for r in want_rgb]
    task = AprilTags(w, h, layout, calib, r2c, cam_id=2, max_batch=n, fourcc="RGB3")
    out, v = task.process_raw_batch([R.pack(c, "RGB3") for c in rgb], gyros)
    assert np.array_equal(v, valid_rgb) and valid_rgb.all() and [bytes(r) for r in out] == want_rgb
    task.detector.close()
    plain.detector.close()


def test_device_frames_equal_host_frames(built):
    """ck_upload_raw_device from a torch tensor — 16-byte aligned with an aligned stride, and with an odd stride at an odd offset —
    stages what ck_upload_raw stages, for every family and orientation."""
    import torch
    from chalkydri_amd.detector import AprilTagDetector
    W, H, n = 272, 200, 3
    det = AprilTagDetector(W, H, max_batch=n)
    rng = np.random.default_rng(77)
    for fourcc in R.FAMILIES:
        for o in R.ORIENTATIONS:
            sw, sh = R.source_size(W, H, o)
            for extra, off in ((0, 0), (16, 0), (5, 0), (0, 3), (7, 9)):
                stride = (R.min_stride(fourcc, sw) + 15) // 16 * 16 + extra if extra in (0, 16) and off == 0 else R.min_stride(fourcc, sw) + extra
                imgs = [rng.integers(0, 256, (sh, sw, 3) if R.is_colour(fourcc) else (sh, sw), dtype=np.uint8) for _ in range(n)]
                packed = [R.pack(im, fourcc, stride, seed=i) for i, im in enumerate(imgs)]
                host_luma = det.raw_luma(packed, fourcc, o).copy()
                pitch = packed[0].size + (0 if off == 0 and extra in (0, 16) else 13)
                flat = np.full(off + n * pitch + 64, 0x3C, np.uint8)
                for i, p in enumerate(packed):
                    flat[off + i * pitch: off + i * pitch + p.size] = p.reshape(-1)
                dev = torch.from_numpy(flat).cuda()
                torch.cuda.synchronize()
                assert dev.data_ptr() % 16 == 0
                det.upload(np.zeros((n, H, W), np.uint8))                       # what is staged now is not the answer
                assert det.upload_raw_device(dev.data_ptr() + off, n, stride, pitch, fourcc, o) == n
                got = S.staged(det, n)
                assert np.array_equal(got, host_luma), (fourcc, o, extra, off, int((got != host_luma).sum()))
    det.close()


def test_raw_ingest_ring_matches_the_plain_path(built):
    """Two raw slots, the second submitted while the first is processed (as test_ring_matches_upload_path): the records of the
    plain upload path.  Slot 0 is filled through ck_ingest_write from camera buffers with a larger stride, slot 1 in place."""
    from chalkydri_amd._lib import ChalkydriError
    from chalkydri_amd.apriltags import AprilTags
    from chalkydri_amd.detector import IngestRing, fourcc as cc
    n = 4
    frames, gyros, layout, r2c, calib = wall_frames(2 * n)
    h, w = frames.shape[1:]
    task = AprilTags(w, h, layout, calib, r2c, cam_id=2, max_batch=n)
    want = [task.process_batch(frames[b * n:(b + 1) * n], gyros[b * n:(b + 1) * n]) for b in range(2)]
    want = [([bytes(r) for r in recs], v.copy()) for recs, v in want]
    want_dets = keys(task.detector.detect_batch(frames[n:]))
    for fourcc, o in (("YUYV", "none"), ("UYVY", "rotate-180"), ("NV12", "none")):
        ring = IngestRing(task.detector, n_slots=2, fourcc=fourcc, orientation=o)
        ms = R.min_stride(fourcc, w)
        assert ring.stride >= ms and ring.stride % 16 == 0 and ring.min_stride == ms
        view = ring.slot_view(1)
        assert view.shape == (n, h, ring.stride)
        src = [R.source_of(f, o) for f in frames]
        for i in range(n):
            ring.write(0, i, R.pack(src[i], fourcc, ms + 24, pad_byte=0xAB, seed=i)[:h])
            view[i, :, :ms] = R.pack(src[n + i], fourcc, seed=i)[:h]
        ring.submit(0, n)
        ring.submit(1, n)
        for b in range(2):
            out, valid = ring.process(b, n, task._pp, gyros[b * n:(b + 1) * n], np.ones(n, np.uint8))
            assert np.array_equal(valid.astype(bool), want[b][1]) and valid.all()
            assert [bytes(r) for r in out] == want[b][0], (fourcc, o, b)
        with pytest.raises(ChalkydriError) as e:
            ring.detect(1, n - 1)
        assert e.value.code == A.CK_EINVAL
        dets, status = ring.detect(1, n)
        assert keys(dets) == want_dets
        # exactly the ring's family: another raw format is refused, a wrong geometry is invalid
        other = "UYVY" if fourcc != "UYVY" else "YUYV"
        arr = (A.ImageU8 * 1)()
        buf = R.pack(src[0], other)
        arr[0].buf, arr[0].width, arr[0].height, arr[0].stride = buf.ctypes.data, w, h, buf.shape[1]
        assert task.detector._L.ck_ingest_write(ring._g, 0, 0, arr, cc(other)) == A.CK_EUNSUPPORTED
        assert task.detector._L.ck_ingest_write(ring._g, 0, 0, arr, cc("MJPG")) == A.CK_EUNSUPPORTED
        arr[0].width = w - 2
        assert task.detector._L.ck_ingest_write(ring._g, 0, 0, arr, cc(fourcc)) == A.CK_EINVAL
        ring.close()
    # a quarter turn: the ring's slots have the source geometry, the handle the turned one
    turned = AprilTags(h, w, layout, calib, r2c, cam_id=2, max_batch=n)
    tw = keys(turned.detector.detect_batch(np.stack([R.orient_vec(f, "clockwise") for f in frames[:n]])))
    ring = IngestRing(turned.detector, n_slots=1, fourcc="YUYV", orientation="clockwise")
    assert ring.slot_view(0).shape == (n, h, ring.stride) and ring.sw == w
    for i in range(n):
        ring.write(0, i, R.pack(frames[i], "YUYV"))
    ring.submit(0, n)
    assert keys(ring.detect(0, n)[0]) == tw
    ring.close()
    turned.detector.close()
    task.detector.close()


def settings_check():
    """quad_decimate 2 and quad_sigma 0.8 behind a raw upload equal the same settings behind ck_upload_frames; a handle that
    served raw calls returns from a plain detect_batch what an untouched handle returns."""
    from chalkydri_amd.detector import AprilTagDetector
    n = 2
    frames, _, _, _, _ = wall_frames(n)
    h, w = frames.shape[1:]
    src = [R.pack(f, "YUYV", R.min_stride("YUYV", w) + 5, seed=1) for f in frames]
    rgb = [R.grey_to_rgb(f, seed=i) for i, f in enumerate(frames)]
    for kw in ({}, {"quad_decimate": 2}, {"quad_sigma": 0.8}, {"quad_decimate": 2, "quad_sigma": 0.8}):
        fresh = AprilTagDetector(w, h, max_batch=n, **kw)
        want = keys(fresh.detect_batch(frames))
        want_q = fresh.quad_image(frames)
        fresh.close()
        det = AprilTagDetector(w, h, max_batch=n, **kw)
        det.upload_raw(src, "YUYV")
        assert keys(det.detect_batch(None, n=n)) == want, kw
        assert np.array_equal(det.quad_image(None, n=n), want_q), kw
        det.upload_raw([R.pack(c, "BGRA") for c in rgb], "BGRA")
        det.detect_batch(None, n=n)
        det.raw_luma([R.pack(R.source_of(f, "rotate-180"), "UYVY") for f in frames], "UYVY", "rotate-180")
        assert keys(det.detect_batch(frames)) == want, kw               # the plain path on a handle that served raw calls
        det.close()
    return True


def test_settings_behind_a_raw_upload(built):
    assert settings_check()


def test_misuse_is_refused_and_the_handle_stays_usable(built):
    from chalkydri_amd.detector import AprilTagDetector, IngestRing, fourcc as cc
    W, H, nb = 64, 48, 2
    det = AprilTagDetector(W, H, max_batch=nb)
    L, h = det._L, det._h
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    good = R.pack(img, "YUYV")
    want = R.expected(good, "YUYV", W, H, good.shape[1], "none")

    def imgs(buf, w, h_, stride, n=1):
        arr = (A.ImageU8 * n)()
        for i in range(n):
            arr[i].buf, arr[i].width, arr[i].height, arr[i].stride = (buf.ctypes.data if buf is not None else None), w, h_, stride
        return arr

    def fmt(code, o=0):
        return C.byref(A.RawFormat(cc(code), o))

    def still_fine():
        assert np.array_equal(det.raw_luma([good], "YUYV")[0], want)

    out = np.empty((nb + 1, H, W), np.uint8)
    ok = imgs(good, W, H, good.shape[1])
    assert L.ck_upload_raw(h, ok, 1, fmt("MJPG")) == A.CK_EUNSUPPORTED; still_fine()
    assert L.ck_upload_raw(h, ok, 1, fmt("YUYV", 4)) == A.CK_EINVAL; still_fine()
    assert L.ck_upload_raw(h, ok, 1, None) == A.CK_EINVAL; still_fine()
    assert L.ck_upload_raw(h, imgs(good, W, H, good.shape[1] - 1), 1, fmt("YUYV")) == A.CK_EINVAL; still_fine()
    assert L.ck_raw_luma_batch(h, imgs(good, W, H, good.shape[1] - 1), 1, fmt("YUYV"), out.ctypes.data) == A.CK_EINVAL; still_fine()
    # a quarter turn takes the TRANSPOSED source geometry: H x W frames for a W x H handle
    assert L.ck_upload_raw(h, ok, 1, fmt("YUYV", A.CK_ORIENT_CLOCKWISE)) == A.CK_EINVAL; still_fine()
    assert L.ck_upload_raw(h, imgs(good, H, W, 2 * H), 1, fmt("YUYV")) == A.CK_EINVAL; still_fine()
    assert L.ck_upload_raw(h, imgs(good, W, H, good.shape[1], nb + 1), nb + 1, fmt("YUYV")) == A.CK_ECAPACITY; still_fine()
    assert L.ck_upload_raw(h, imgs(None, W, H, good.shape[1]), 1, fmt("YUYV")) == A.CK_EINVAL; still_fine()
    assert L.ck_upload_raw(h, None, 1, fmt("YUYV")) == A.CK_EINVAL; still_fine()
    assert L.ck_upload_raw(h, ok, -1, fmt("YUYV")) == A.CK_EINVAL; still_fine()
    assert L.ck_raw_luma_batch(h, ok, 1, fmt("YUYV"), None) == A.CK_EINVAL; still_fine()
    assert L.ck_upload_raw_device(h, None, 1, good.shape[1], good.size, fmt("YUYV")) == A.CK_EINVAL; still_fine()
    assert L.ck_upload_raw_device(h, C.c_void_p(16), 1, good.shape[1] - 1, good.size, fmt("YUYV")) == A.CK_EINVAL; still_fine()
    assert L.ck_upload_raw_device(h, C.c_void_p(16), 1, good.shape[1], good.size - 1, fmt("YUYV")) == A.CK_EINVAL; still_fine()
    assert L.ck_upload_raw_device(h, C.c_void_p(16), nb + 1, good.shape[1], good.size, fmt("YUYV")) == A.CK_ECAPACITY; still_fine()
    assert L.ck_upload_raw_device(h, C.c_void_p(16), 1, good.shape[1], good.size, fmt("H264")) == A.CK_EUNSUPPORTED; still_fine()
    g = C.c_void_p()
    assert L.ck_ingest_create_raw(h, 2, fmt("MJPG"), C.byref(g)) == A.CK_EUNSUPPORTED and not g.value
    assert L.ck_ingest_create_raw(h, 2, fmt("YUYV", -1), C.byref(g)) == A.CK_EINVAL and not g.value
    assert L.ck_ingest_create_raw(h, 2, None, C.byref(g)) == A.CK_EINVAL and not g.value
    assert L.ck_ingest_create_raw(h, 9, fmt("YUYV"), C.byref(g)) == A.CK_EINVAL and not g.value
    # a ring of ck_ingest_create is the ring of before: YUYV is refused, GREY is taken
    ring = IngestRing(det, n_slots=1)
    assert L.ck_ingest_write(ring._g, 0, 0, imgs(good, W, H, good.shape[1]), cc("YUYV")) == A.CK_EUNSUPPORTED
    assert L.ck_ingest_write(ring._g, 0, 0, imgs(img, W, H, W), cc("GREY")) == A.CK_OK
    assert ring.stride == det.cfg.width and ring.slot_view(0).shape == (nb, H, W)
    ring.close()
    # n = 0 stages nothing and is no error
    assert L.ck_upload_raw(h, None, 0, fmt("YUYV")) == A.CK_OK; still_fine()
    det.close()


def test_stress_helping(built):
    out = S.run(40, 7)
    assert out["mismatching"] == 0 and out["device_cases"] == 10, out

