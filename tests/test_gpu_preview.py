"""JPEG preview of the staged frames on the GPU (ck_preview_jpeg / ck_preview_luma): the scaled (+ overlaid)
pixels and the complete files byte-equal to the numpy restatement (tests/np_jpeg_enc.py), which tests/test_jpeg_enc_host.py ties
to libjpeg; truncation, device output, index lists, the workspace left untouched, and the misuse cases of the contract."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg as J  # noqa: E402
import np_jpeg_enc as E  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

HANDLES = [(1280, 800), (640, 480), (641, 479), (272, 200)]
QUALITIES = [1, 20, 50, 85, 100]
RESTARTS = [0, 1, 3]


def previews(W, H):
    """(width, height) requests: 640 x 480 (clipped on a smaller handle), W x H, 320 x 200, 8 x 8, 333 x 77"""
    return [(640, 480), (0, 0), (320, 200), (8, 8), (333, 77)]


def extremes(h, w):
    """The blocks that stress the FDCT's range, in quadrants: all 0, all 255, 0/255 checkerboard, single bright pixels."""
    f = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    f[:h // 2, w // 2:] = 255
    f[h // 2:, :w // 2] = (((xx + yy) % 2) * 255)[h // 2:, :w // 2]
    f[h // 2:, w // 2:] = np.where((xx % 8 == 3) & (yy % 8 == 5), 255, 0)[h // 2:, w // 2:]
    return f


def contents(W, H, seed):
    from chalkydri_amd import scenes
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    scene = scenes.bench_stream(seed, 1, W, H, 4)[0][0]
    return np.stack([scene, rng.integers(0, 256, (H, W)).astype(np.uint8), extremes(H, W), (((xx + yy + 1) % 2) * 255).astype(np.uint8)])


def detector(w, h, nb, **kw):
    from chalkydri_amd.detector import AprilTagDetector
    return AprilTagDetector(w, h, max_batch=nb, **kw)


def rc_of(call):
    from chalkydri_amd._lib import ChalkydriError
    try:
        call()
    except ChalkydriError as e:
        return e.code
    return A.CK_OK


@pytest.mark.parametrize("W,H", HANDLES)
def test_luma_and_files_equal_the_restatement(built, W, H):
    """Every handle x preview geometry x quality x restart_rows on a scene, noise and the extreme blocks: preview_luma equals
    scale_nn and preview_jpeg equals encode_grey (hence libjpeg) byte for byte."""
    F = contents(W, H, W + H)
    det = detector(W, H, len(F))
    det.upload(F)
    bad = []
    for width, height in previews(W, H):
        pw, ph, _ = E.layout(width, height, W, H)
        want = [E.scale_nn(f, pw, ph) for f in F]
        got = det.preview_luma(n=len(F), width=width, height=height)
        assert got.shape == (len(F), ph, pw)
        for i in range(len(F)):
            assert np.array_equal(got[i], want[i]), (width, height, i)
        for q in QUALITIES:
            for rr in RESTARTS:
                files = det.preview_jpeg(n=len(F), width=width, height=height, quality=q, restart_rows=rr)
                for i in range(len(F)):
                    if files[i] != E.encode_grey(want[i], q, rr):
                        bad.append((width, height, q, rr, i, len(files[i])))
    det.close()
    assert not bad, (len(bad), bad[:10])


def test_luma_after_jpeg_and_raw_uploads(built):
    """The preview reads the staged frames whatever staged them: a JPEG upload, a raw upload with a quarter turn."""
    W, H = 272, 200
    rng = np.random.default_rng(5)
    F = contents(W, H, 11)[:2]
    det = detector(W, H, 2)
    streams = [J.encode(f, sampling="420", quality=90) for f in F]
    det.upload_jpeg(streams)
    for width, height in previews(W, H):
        pw, ph, _ = E.layout(width, height, W, H)
        got = det.preview_luma(n=2, width=width, height=height)
        for i in range(2):
            assert np.array_equal(got[i], E.scale_nn(J.decode_luma(streams[i])[0], pw, ph)), (width, height, i)
    raw = [np.ascontiguousarray(rng.integers(0, 256, (W, 2 * H)).astype(np.uint8)) for _ in range(2)]   # YUYV, source H x W
    staged = det.raw_luma(raw, "YUYV", "clockwise")
    for width, height in previews(W, H):
        pw, ph, _ = E.layout(width, height, W, H)
        got = det.preview_luma(n=2, width=width, height=height)
        files = det.preview_jpeg(n=2, width=width, height=height, quality=85, restart_rows=1)
        for i in range(2):
            assert np.array_equal(got[i], E.scale_nn(staged[i], pw, ph)), (width, height, i)
            assert files[i] == E.encode_grey(got[i], 85, 1)
    det.close()


def test_index_list_repeats_and_reorders(built):
    """A batch of max_batch entries whose index list repeats and reorders frames gives, per entry, the bytes of a one-frame call."""
    W, H, nb = 640, 480, 8
    from chalkydri_amd import scenes
    F = scenes.bench_stream(3, 5, W, H, 4)[0]
    det = detector(W, H, nb)
    det.upload(F)
    idx = [4, 0, 0, 3, 1, 4, 2, 0]
    for kw in ({}, {"width": 0, "height": 0, "quality": 85, "restart_rows": 3}):
        files = det.preview_jpeg(idx, **kw)
        luma = det.preview_luma(idx, **kw)
        for k, f in enumerate(idx):
            assert files[k] == det.preview_jpeg([f], **kw)[0], (k, f)
            assert np.array_equal(luma[k], det.preview_luma([f], **kw)[0])
    det.close()


def test_overlay_equals_the_restatement(built):
    """After detect_uploaded on rendered scenes the overlaid pixels equal the restatement applied to the returned detections and
    the JPEG equals their encoding; the detections and the poses are what they were before the preview calls."""
    from chalkydri_amd import scenes
    from chalkydri_amd.detector import tag_pose_params
    W, H, n = 1280, 800, 4
    F = scenes.bench_stream(7, n, W, H, 6)[0]
    det = detector(W, H, n)
    det.upload(F)
    dets = det.detect_batch(None, n=n)
    assert sum(len(d) for d in dets) > 0
    pp = tag_pose_params(900.0, 900.0, W / 2, H / 2)
    poses0 = [[bytes(r) for r in fr] for fr in det.last_tag_poses(pp, raw=True)]
    for width, height in [(640, 480), (0, 0), (333, 77)]:
        pw, ph, _ = E.layout(width, height, W, H)
        idx = [2, 0, 3, 1]
        luma = det.preview_luma(idx, width=width, height=height, overlay=True)
        files = det.preview_jpeg(idx, width=width, height=height, overlay=True, restart_rows=1)
        plain = det.preview_luma(idx, width=width, height=height)
        for k, f in enumerate(idx):
            want = E.preview(F[f], pw, ph, [d.corners() for d in dets[f]])
            assert np.array_equal(luma[k], want), (width, height, f, int((luma[k] != want).sum()))
            assert len(dets[f]) == 0 or not np.array_equal(luma[k], plain[k])
            assert files[k] == E.encode_grey(want, 50, 1)
    # the workspace and the staged frames are untouched
    assert [[bytes(r) for r in fr] for fr in det.last_tag_poses(pp, raw=True)] == poses0
    again = det.detect_batch(None, n=n)
    assert [[(d.id(), d.corners().tobytes()) for d in fr] for fr in again] == [[(d.id(), d.corners().tobytes()) for d in fr] for fr in dets]
    det.close()


def test_overlay_needs_a_valid_detection_result(built):
    W, H = 640, 480
    from chalkydri_amd import scenes
    F = scenes.bench_stream(2, 3, W, H, 4)[0]
    det = detector(W, H, 3)
    det.upload(F)
    assert rc_of(lambda: det.preview_jpeg(n=1, overlay=True)) == A.CK_EINVAL          # nothing detected yet
    assert rc_of(lambda: det.preview_luma(n=1, overlay=True)) == A.CK_EINVAL
    det.detect_batch(None, n=2)
    assert len(det.preview_jpeg(n=2, overlay=True)) == 2
    assert rc_of(lambda: det.preview_jpeg([2], overlay=True)) == A.CK_EINVAL          # staged, but the detect call did not cover it
    assert len(det.preview_jpeg([2])) == 1
    det.quads(F[:1])                                                                  # rewrites the workspace
    assert rc_of(lambda: det.preview_jpeg(n=1, overlay=True)) == A.CK_EINVAL
    det.close()


def test_round_trip_through_the_decoder(built):
    """upload_jpeg(preview bytes) on a handle of the preview's size stages exactly np_jpeg.decode_luma(bytes)."""
    W, H = 640, 480
    F = contents(W, H, 21)[:3]
    det = detector(W, H, 3)
    det.upload(F)
    for (pw, ph), q, rr in [((320, 200), 50, 0), ((333, 77), 85, 1), ((640, 480), 20, 3)]:
        files = det.preview_jpeg(n=3, width=pw, height=ph, quality=q, restart_rows=rr)
        small = detector(pw, ph, 3)
        got, st = small.decode_jpeg(files, return_status=True)
        for i in range(3):
            want, wst = J.decode_luma(files[i])
            assert wst == J.OK and st[i] == A.CK_JPEG_OK
            assert np.array_equal(got[i], want), (pw, ph, q, rr, i)
        small.close()
    det.close()


def test_truncation_and_device_output(built):
    """cap_per_frame too small: CK_OK, CK_PREVIEW_TRUNCATED, the true size, nothing written past a slot, the other frames intact;
    a device `out` pointer gives the same bytes as a host one."""
    import torch
    W, H, n = 640, 480, 4
    F = contents(W, H, 31)
    det = detector(W, H, n)
    det.upload(F)
    full = det.preview_jpeg(n=n, width=320, height=200, quality=50)
    sizes_full = [len(b) for b in full]
    cap = sorted(sizes_full)[1] + 1          # at least one file fits, at least one does not
    assert any(s > cap for s in sizes_full) and any(s <= cap for s in sizes_full)
    pp = __import__("chalkydri_amd.detector", fromlist=["preview_params"]).preview_params(320, 200, 50)
    # out is [n][cap]: the byte behind slot i is slot i + 1's first byte (checked to be that file's), the byte behind the last
    # slot is a canary, and so is every byte of a slot behind a file that fits
    flat = np.full(n * cap + 1, 0xC3, np.uint8)
    sizes, status = (C.c_int64 * n)(), (C.c_uint32 * n)()
    assert det._L.ck_preview_jpeg(det._h, C.byref(pp), None, n, flat.ctypes.data, cap, sizes, status) == A.CK_OK
    assert flat[n * cap] == 0xC3
    for i in range(n):
        assert sizes[i] == sizes_full[i]
        assert status[i] == (A.CK_PREVIEW_TRUNCATED if sizes_full[i] > cap else A.CK_PREVIEW_OK)
        used = min(cap, sizes_full[i])
        assert flat[i * cap:i * cap + used].tobytes() == full[i][:used]
        if used < cap:   # the rest of a slot whose file fits is not written
            assert np.all(flat[i * cap + used:(i + 1) * cap] == 0xC3)
    # the same call into device memory, canaries behind every byte the call may write
    dev = torch.full((n * cap + 64,), 0xC3, dtype=torch.uint8, device="cuda")
    sizes2, status2 = (C.c_int64 * n)(), (C.c_uint32 * n)()
    assert det._L.ck_preview_jpeg(det._h, C.byref(pp), None, n, C.c_void_p(dev.data_ptr()), cap, sizes2, status2) == A.CK_OK
    torch.cuda.synchronize()
    host = dev.cpu().numpy()
    assert np.array_equal(host[:n * cap], flat[:n * cap]) and np.all(host[n * cap:] == 0xC3)
    assert list(sizes2) == list(sizes) and list(status2) == list(status)
    # python surface: the files come back cut to cap with their status
    files, sz, st = det.preview_jpeg(n=n, width=320, height=200, quality=50, cap=cap, return_status=True)
    assert sz == sizes_full and [len(b) for b in files] == [min(cap, s) for s in sizes_full] and st == list(status)
    det.close()


def test_misuse(built):
    """Every error of the contract, with the call's arguments otherwise valid."""
    from chalkydri_amd.detector import preview_params
    W, H, nb = 272, 200, 2
    det = detector(W, H, nb)
    L, h = det._L, det._h
    good = preview_params()
    _, _, mb = E.layout(640, 480, W, H)
    out = np.zeros(nb * mb, np.uint8)
    sizes, status = (C.c_int64 * 4)(), (C.c_uint32 * 4)()
    idx = (C.c_int32 * 4)(0, 1, 0, 1)

    def jpeg(pp=good, frames=None, n=1, o=out.ctypes.data, cap=mb, s=sizes, hh=h):
        return L.ck_preview_jpeg(hh, C.byref(pp) if pp is not None else None, frames, n, o, cap, s, status)

    def luma(pp=good, frames=None, n=1, o=out.ctypes.data, hh=h):
        return L.ck_preview_luma(hh, C.byref(pp) if pp is not None else None, frames, n, o)
    assert jpeg() == A.CK_EINVAL and luma() == A.CK_EINVAL                       # nothing staged yet
    assert jpeg(n=0) == A.CK_OK and luma(n=0) == A.CK_OK
    det.upload(contents(W, H, 1)[:2])
    assert jpeg(n=2) == A.CK_OK and luma(n=2) == A.CK_OK
    assert jpeg(hh=None) == A.CK_EINVAL and luma(hh=None) == A.CK_EINVAL
    assert jpeg(pp=None) == A.CK_EINVAL and luma(pp=None) == A.CK_EINVAL
    assert jpeg(o=None) == A.CK_EINVAL and luma(o=None) == A.CK_EINVAL
    assert jpeg(s=None) == A.CK_EINVAL
    assert jpeg(n=-1) == A.CK_EINVAL and luma(n=-1) == A.CK_EINVAL
    assert jpeg(cap=0) == A.CK_EINVAL
    assert jpeg(n=3, frames=idx) == A.CK_ECAPACITY and luma(n=3, frames=idx) == A.CK_ECAPACITY
    assert jpeg(n=2, frames=idx) == A.CK_OK
    for bad in ((C.c_int32 * 2)(0, 2), (C.c_int32 * 2)(-1, 0)):
        assert jpeg(n=2, frames=bad) == A.CK_EINVAL and luma(n=2, frames=bad) == A.CK_EINVAL
    det.upload(contents(W, H, 1)[:1])                                             # one frame staged now: index 1 is stale
    assert jpeg(n=2) == A.CK_EINVAL and jpeg(n=1) == A.CK_OK
    for kw in ({"width": 7}, {"height": 7}, {"width": -1}, {"height": -8}, {"quality": 0}, {"quality": 101}, {"restart_rows": -1},
               {"restart_rows": 65536 // 34 + 1, "width": 0, "height": 0}):
        pp = preview_params(**kw)
        assert jpeg(pp=pp) == A.CK_EINVAL and luma(pp=pp) == A.CK_EINVAL, kw
    pp = preview_params()
    pp.overlay = 2
    assert jpeg(pp=pp) == A.CK_EINVAL
    assert jpeg(pp=preview_params(restart_rows=65535 // 34, width=0, height=0)) == A.CK_OK   # DRI = 34 * 1927 <= 65535
    det.close()


def test_stress_helping(built):
    """A small helping of tests/stress_preview.py (random geometry, quality, restart rows, content, overlay, index lists)."""
    import stress_preview
    r = stress_preview.run(24, 5)
    assert r["mismatching"] == 0, r


def test_poison_mode(built):
    """The same helping in a child whose handles start as 0xA5 bytes (CK_POISON=1): nothing is read that the call did not write."""
    env = dict(os.environ, CK_POISON="1")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "stress_preview.py"), "16", "9"],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '"mismatching": 0' in r.stdout, r.stdout[-2000:]
