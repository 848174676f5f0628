"""Exposure metering on the device: ck_exposure_stats byte-equal to the numpy restatement (tests/np_exposure.py)
fed the library's own tables, over sizes, contents, rectangles and frame lists; the same after every route into the staged
frames; no interference with detection; misuse refused; the closed loop driven by device statistics equal to the numpy-driven
one; AprilTags(auto_exposure=True)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_exposure as N  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = ((640, 480), (641, 479), (272, 200), (16, 16), (1280, 800))


def _contents(w, h, seed):
    """Frames of one size: noise of amplitude 0 (flat), 1, 4, 16 around different levels, full-range noise, all 0, all 255."""
    rng = np.random.default_rng(seed)
    out = []
    for amp, base in ((0, 77), (1, 3), (4, 128), (16, 200), (16, 8)):
        out.append(np.clip(base + rng.integers(-amp, amp + 1, (h, w)), 0, 255).astype(np.uint8))
    out.append(rng.integers(0, 256, (h, w), dtype=np.uint8))
    out.append(np.zeros((h, w), np.uint8))
    out.append(np.full((h, w), 255, np.uint8))
    return np.stack(out)


def _rois(w, h):
    return [None, (w // 4, h // 4, 3 * w // 4, 3 * h // 4), (0, 3, w // 2, h - 2), (2, 0, w - 3, h // 2), (w // 2, 1, w, h - 1),
            (1, h // 2, w - 1, h), (-50, -50, w + 50, h + 50), (5, 5, 5, 9), (w + 3, 2, w + 9, 8), (7, 9, 8, 10), (0, 0, 1, h), (w - 1, 0, w, h)]


def _check(got, frames, lut, rois, idx=None):
    idx = range(len(got)) if idx is None else idx
    for i, f in enumerate(idx):
        roi = rois[i] if isinstance(rois, list) else rois
        want = N.stats(frames[f], lut, roi)
        assert got[i].tobytes() == want.tobytes(), (i, f, roi)
        x0, y0, x1, y1 = N.clamp_roi(roi, frames.shape[2], frames.shape[1])
        area = max(x1 - x0, 0) * max(y1 - y0, 0)
        assert int(got[i]["luma"].sum()) == int(got[i]["n_luma"]) == area
        assert all(int(got[i]["grad"][k].sum()) == int(got[i]["n_grad"]) for k in range(N.GAMMAS))


@pytest.mark.parametrize("w,h", SIZES)
def test_stats_equal_the_restatement(built, w, h):
    from chalkydri_amd.detector import AprilTagDetector
    from chalkydri_amd.exposure import ExposureParams
    frames = _contents(w, h, w * 31 + h)
    n = len(frames)
    det = AprilTagDetector(w, h, max_batch=n)
    lut = ExposureParams().luts()
    det.upload(frames)
    _check(det.exposure_stats(n=n), frames, lut, None)
    rois = _rois(w, h)
    for r0 in range(0, len(rois), n):                      # a rectangle per frame, every rectangle on some frame
        rr = [rois[(r0 + i) % len(rois)] for i in range(n)]
        got = det.exposure_stats(n=n, roi=[(0, 0, w, h) if r is None else r for r in rr])
        _check(got, frames, lut, rr)
    perm = [5, 0, 7, 2, 2, 6]                              # a permuted list with a repeat
    _check(det.exposure_stats(frames=perm, roi=rois[1]), frames, lut, rois[1], perm)
    _check(det.exposure_stats(n=3), frames, lut, None)     # fewer than are staged
    assert det.exposure_stats(n=0).shape == (0,)
    # other gamma curves, the library's tables for them
    p = ExposureParams(gamma=(0.2, 0.4, 0.7, 0.9, 1.0, 2.5, 4.0))
    _check(det.exposure_stats(n=n, params=p), frames, p.luts(), None)
    a = det.exposure_stats(n=n, roi=rois[1])
    assert a.tobytes() == det.exposure_stats(n=n, roi=rois[1]).tobytes()      # metering twice
    det.close()


def test_every_ingest_path_and_no_interference(built):
    import np_jpeg_enc as E
    import scenes
    from chalkydri_amd.detector import AprilTagDetector, IngestRing
    from chalkydri_amd.exposure import ExposureParams
    w, h, n = 320, 240, 3
    frames = scenes.bench_stream(5, n, w, h, 4)[0]
    lut = ExposureParams().luts()
    det = AprilTagDetector(w, h, max_batch=n)
    # detection with and without metering in between: the same bytes
    det.upload(frames)
    want = [[(d.id(), d.corners().tobytes(), d.decision_margin()) for d in fr] for fr in det.detect_batch(None, n=n)]
    assert any(want)
    det.upload(frames)
    s0 = det.exposure_stats(n=n)
    got = [[(d.id(), d.corners().tobytes(), d.decision_margin()) for d in fr] for fr in det.detect_batch(None, n=n)]
    assert got == want
    _check(s0, frames, lut, None)
    _check(det.exposure_stats(n=n), frames, lut, None)     # after detection the staged frames are still what they were
    # strided host views
    wide = np.zeros((n, h, w + 13), np.uint8)
    wide[:, :, :w] = frames
    arr = (A.ImageU8 * n)()
    for i in range(n):
        arr[i].buf, arr[i].width, arr[i].height, arr[i].stride = wide[i].ctypes.data, w, h, w + 13
    assert det._L.ck_upload_frames(det._h, arr, n) == 0
    _check(det.exposure_stats(n=n), frames, lut, None)
    # upload_raw: YUYV with a quarter turn (the source is h x w, its luma turned clockwise is the frame)
    src = np.stack([np.rot90(f, 1) for f in frames])        # clockwise(src) == frame
    yuyv = np.zeros((n, w, 2 * h), np.uint8)
    yuyv[:, :, 0::2] = src
    yuyv[:, :, 1::2] = 128
    det.upload_raw(list(yuyv), "YUYV", "clockwise")
    staged = det.quad_image(None, n=n)
    _check(det.exposure_stats(n=n), staged, lut, None)
    # upload_jpeg with an orientation: whatever the decoder staged is what is metered
    jp = [E.encode_grey(np.ascontiguousarray(np.rot90(f, 2)), 90, 0) for f in frames]
    det.upload_jpeg(jp, "rotate-180")
    staged = det.quad_image(None, n=n)
    _check(det.exposure_stats(n=n, roi=(10, 20, 300, 200)), staged, lut, (10, 20, 300, 200))
    # a slot of the JPEG ingest ring
    ring = IngestRing(det, n_slots=2, fourcc="MJPG", orientation="rotate-180")
    for i in range(n):
        ring.write(1, i, jp[i])
    ring.submit(1, n)
    rs = ring.exposure_stats(1, frames=[2, 0, 1])
    _check(rs, staged, lut, None, [2, 0, 1])
    d_ring, _ = ring.detect(1, n)
    det.upload_jpeg(jp, "rotate-180")
    assert [[d.id() for d in fr] for fr in d_ring] == [[d.id() for d in fr] for fr in det.detect_batch(None, n=n)]
    ring.close()
    det.close()


def test_process_uploaded_is_untouched_and_auto_exposure(built):
    import scenes
    from chalkydri_amd.apriltags import AprilTags
    w, h, n = 640, 480, 2
    frames, gyro, layout, calib, r2c = scenes.bench_stream(1, n, w, h, 4)
    off = AprilTags(w, h, layout, calib, r2c, cam_id=1, max_batch=n)
    on = AprilTags(w, h, layout, calib, r2c, cam_id=1, max_batch=n, auto_exposure=True, exposure0=10.0)
    r0, v0 = off.process_batch(frames, list(gyro))
    r1, v1 = on.process_batch(frames, list(gyro))
    assert [bytes(r) for r in r0] == [bytes(r) for r in r1] and np.array_equal(v0, v1) and v0.any()
    assert off.exposure is None
    from chalkydri_amd.exposure import ExposureParams, recommend
    want, _ = recommend(N.stats(frames[n - 1], ExposureParams().luts()), 10.0)
    assert on.exposure == want and on.exposure > 0
    # process after metering by hand returns what it returns without
    off.detector.upload(frames)
    off.detector.exposure_stats(n=n)
    r2, v2 = off.process_batch(None, list(gyro), n=n)
    assert [bytes(r) for r in r0] == [bytes(r) for r in r2] and np.array_equal(v0, v2)


def test_misuse_is_refused(built):
    from chalkydri_amd.detector import AprilTagDetector
    from chalkydri_amd.exposure import ExposureParams
    w, h, n = 320, 240, 2
    det = AprilTagDetector(w, h, max_batch=4)
    L, hd = det._L, det._h
    frames = _contents(w, h, 3)[:n]
    det.upload(frames)
    p = ExposureParams()
    out = (A.ExposureStats * 8)()
    idx = (C.c_int32 * 4)(0, 1, 0, 1)
    call = lambda h_=hd, f=None, n_=n, pp=C.byref(p.c), roi=None, o=out: L.ck_exposure_stats(h_, f, n_, pp, roi, o)
    assert call() == 0
    assert call(h_=None) == A.CK_EINVAL and call(pp=None) == A.CK_EINVAL and call(o=None) == A.CK_EINVAL
    assert call(n_=-1) == A.CK_EINVAL and call(n_=n + 1) == A.CK_EINVAL          # more than are staged
    assert call(n_=5) in (A.CK_EINVAL, A.CK_ECAPACITY)                           # more than the handle holds
    idx[3] = n
    assert call(f=idx, n_=4) == A.CK_EINVAL                                      # an index beyond what is staged
    idx[3] = -1
    assert call(f=idx, n_=4) == A.CK_EINVAL
    idx[3] = 1
    assert call(f=idx, n_=4) == 0
    for field, v in (("lambda_", 0.0), ("delta", 1.0), ("kp", float("nan")), ("e_min", 1e9)):
        q = ExposureParams()
        setattr(q.c, field, v)
        assert call(pp=C.byref(q.c)) == A.CK_EINVAL, field
    q = ExposureParams()
    q.c.gamma[3] = q.c.gamma[2]
    assert call(pp=C.byref(q.c)) == A.CK_EINVAL
    assert L.ck_exposure_stats_ingested(None, 0, None, 1, C.byref(p.c), None, out) == A.CK_EINVAL
    lut = p.luts()
    _check(det.exposure_stats(n=n), frames, lut, None)                           # the handle still works
    det.close()


def test_closed_loop_on_the_device(built, oracle):
    """The trajectory driven by device statistics equals the numpy-driven one exactly (the same histograms go into the same C
    function); real detection loses tags at the under-exposed start and finds them all at the end."""
    import exposure_scenes as S
    from chalkydri_amd.detector import AprilTagDetector
    from chalkydri_amd.exposure import ExposureController, ExposureParams
    rad, truth = S.radiance(1)
    e_star = S.best_exposure(rad)
    h, w = rad.shape
    det = AprilTagDetector(w, h, max_batch=1)
    lut = ExposureParams().luts()
    ids = sorted(t["id"] for t in truth)
    for start in (e_star / 8, e_star * 8):
        dev, ref = ExposureController(None, start), ExposureController(None, start)
        for _ in range(2 * S.STEPS):
            det.upload(N.photograph(rad, dev.exposure)[None])
            a = dev.update(det.exposure_stats(n=1))
            b = ref.update(N.stats(N.photograph(rad, ref.exposure), lut))
            assert a == b
        assert abs(np.log(dev.exposure / e_star)) <= 1.5 * S.BAND
        found = lambda e: sorted(d.id() for d in det.detect_batch(N.photograph(rad, e)[None])[0] if d.id() in ids)
        assert found(dev.exposure) == ids
        if start < e_star:
            assert len(found(start)) < len(ids)
    det.close()


def test_the_file_passes_with_poisoned_allocations(built):
    """CK_POISON=1 fills every device allocation with 0xA5: the kernel zeroes what it accumulates into."""
    if os.environ.get("CK_POISON"):
        pytest.skip("already the poisoned run")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "restatement and (16-16 or 641-479 or 272-200) or misuse"],
                       env=dict(os.environ, CK_POISON="1"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
