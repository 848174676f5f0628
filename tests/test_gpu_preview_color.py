"""Colour preview from the raw frames on the GPU (ck_preview_jpeg_color*, ck_preview_color*): the (Y, Cb, Cr)
triples equal tests/preview_color_ref.py and the complete files equal tests/np_jpeg_enc_color.py (which
tests/test_preview_color_host.py ties to libjpeg) byte for byte — through the handle's raw staging, a caller's device memory and
a raw ingest ring; overlay, truncation, and the refusals of the contract."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg_enc as E  # noqa: E402
import np_jpeg_enc_color as EC  # noqa: E402
import preview_color_ref as PC  # noqa: E402
import raw_format_ref as R  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

PREVIEWS = [(0, 0), (8, 8), (40, 24), (37, 21)]   # identity, one MCU, two non-integer ratios with ragged right and bottom blocks


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


_files = {}


def want_file(P, q, rr):
    """encode_ycc, computed once per distinct picture (repeated indices and repeated calls ask for the same files)."""
    key = (P.shape, P.tobytes(), q, rr)
    if key not in _files:
        _files[key] = EC.encode_ycc(P, q, rr)
    return _files[key]


def check_matrix(W, H, families, orientations, previews):
    rng = np.random.default_rng(W * 1000 + H)
    det = detector(W, H, 3)
    idx = [1, 0, 1]
    bad = []
    for fourcc in families:
        for o in orientations:
            sw, sh = R.source_size(W, H, o)
            stride = R.min_stride(fourcc, sw)
            raw = [PC.pack_colour(rng, fourcc, sw, sh) for _ in range(2)]
            staged = det.raw_luma(raw, fourcc, o)
            for width, height in previews:
                pw, ph, _ = EC.layout(width, height, W, H)
                want = [PC.triples_vec(raw[f], fourcc, sw, sh, stride, o, pw, ph) for f in (0, 1)]
                got = det.preview_color(idx, width=width, height=height)
                assert got.shape == (3, ph, pw, 3)
                for rr in (0, 1):
                    files = det.preview_jpeg_color(idx, width=width, height=height, quality=50, restart_rows=rr)
                    for k, f in enumerate(idx):
                        if not np.array_equal(got[k], want[f]) or files[k] != want_file(want[f], 50, rr):
                            bad.append((fourcc, o, width, height, rr, k, bool(np.array_equal(got[k], want[f]))))
            # the luma plane of the colour file is the staged frame (Y is §4d's L)
            assert np.array_equal(det.preview_color([0], width=0, height=0)[0, :, :, 0], staged[0]), (fourcc, o)
    det.close()
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("W,H", [(64, 48), (130, 33), (66, 49)])
def test_triples_and_files_equal_the_restatement(built, W, H):
    """Handles 64 x 48, 130 x 33 and 66 x 49 (a ragged last MCU at identity size) x the four previews x the six families x the
    four orientations x restart_rows 0 and 1, n = 3 with a repeated index, random content."""
    check_matrix(W, H, PC.FAMILIES, R.ORIENTATIONS, PREVIEWS)


def test_half_filled_last_pair_is_sampled(built):
    """A 131-wide 4:2:2 source under the quarter turns: the last pixel's pair has no second pixel, its U and V are read."""
    check_matrix(33, 131, ("YUYV", "UYVY"), ("clockwise", "counterclockwise"), [(0, 0), (8, 8)])


def test_noise_at_the_ends_of_the_quality_range(built):
    """Quality 1 and 100 on noise: byte stuffing in all components and the longest codes of the chrominance tables."""
    W, H = 66, 49
    rng = np.random.default_rng(3)
    det = detector(W, H, 1)
    for fourcc in ("RGB3", "UYVY"):
        raw = [PC.pack_colour(rng, fourcc, W, H)]
        det.upload_raw(raw, fourcc)
        P = PC.triples_vec(raw[0], fourcc, W, H, R.min_stride(fourcc, W), "none", W, H)
        for q in (1, 100):
            for rr in (0, 1):
                f = det.preview_jpeg_color(n=1, width=0, height=0, quality=q, restart_rows=rr)[0]
                assert f == EC.encode_ycc(P, q, rr), (fourcc, q, rr)
                assert q == 1 or f.count(b"\xff\x00") > 0
    det.close()


def test_overlay_in_every_orientation(built):
    """An RGB3 frame whose luma is a rendered tag scene: tags are found, the overlay's triple lies on exactly the restatement's
    pixels, the files equal their encoding; poses, detections and the staged luma are what they were before the calls."""
    from chalkydri_amd import scenes
    from chalkydri_amd.detector import tag_pose_params
    W, H = 640, 480
    frame = scenes.bench_stream(7, 1, W, H, 4)[0][0]
    rgb = R.grey_to_rgb(frame, 1)
    assert np.abs(R.L(rgb[..., 0], rgb[..., 1], rgb[..., 2]).astype(int) - frame).max() <= 2 and (rgb[..., 0] != rgb[..., 2]).any()
    det = detector(W, H, 1)
    pp = tag_pose_params(900.0, 900.0, W / 2, H / 2)
    ovl = np.array(EC.OVERLAY_TRIPLE, np.uint8)
    for o in R.ORIENTATIONS:
        sw, sh = R.source_size(W, H, o)
        raw = R.pack(R.source_of(rgb, o), "RGB3")
        det.upload_raw([raw], "RGB3", o)
        dets = det.detect_batch(None, n=1)
        assert len(dets[0]) > 0, o
        corners = [d.corners() for d in dets[0]]
        poses0 = [[bytes(r) for r in fr] for fr in det.last_tag_poses(pp, raw=True)]
        luma0 = det.quad_image(None, n=1)                       # (quad_decimate 1, no filter: the staged frames, read back as they are)
        assert np.array_equal(luma0[0], R.expected(raw, "RGB3", sw, sh, 3 * sw, o))
        for (width, height), with_file in [((0, 0), False), ((320, 200), True)]:
            pw, ph, _ = EC.layout(width, height, W, H)
            want = PC.triples_vec(raw, "RGB3", sw, sh, 3 * sw, o, pw, ph, corners)
            plain = PC.triples_vec(raw, "RGB3", sw, sh, 3 * sw, o, pw, ph)
            got = det.preview_color(n=1, width=width, height=height, overlay=True)[0]
            assert np.array_equal(got, want), (o, width, int((got != want).any(-1).sum()))
            mask = E.overlay_mask(corners, pw, ph, W, H)
            assert mask.any() and (got[mask] == ovl).all() and np.array_equal(got[~mask], plain[~mask])
            if with_file:
                assert det.preview_jpeg_color(n=1, width=width, height=height, overlay=True, restart_rows=1)[0] == EC.encode_ycc(want, 50, 1)
        assert [[bytes(r) for r in fr] for fr in det.last_tag_poses(pp, raw=True)] == poses0
        assert np.array_equal(det.quad_image(None, n=1), luma0)
        again = det.detect_batch(None, n=1)
        assert [(d.id(), d.corners().tobytes()) for d in again[0]] == [(d.id(), d.corners().tobytes()) for d in dets[0]]
    det.close()


def test_apriltags_preview_in_colour(built):
    """The task layer: after process_raw_batch of a packed colour format, AprilTags.preview(color=True) gives the colour files
    with the tags outlined, preview() the grey ones as before."""
    from chalkydri_amd import scenes
    from chalkydri_amd.apriltags import AprilTags
    W, H, n = 640, 480, 2
    frames, gyro, layout, calib, r2c = scenes.bench_stream(1, n, W, H, 4)
    o = "clockwise"
    sw, sh = R.source_size(W, H, o)
    raw = [R.pack(R.source_of(R.grey_to_rgb(f, 2), o), "BGRA", seed=4) for f in frames]
    task = AprilTags(W, H, layout, calib, r2c, cam_id=1, max_batch=n, fourcc="BGRA", orientation=o)
    task.process_raw_batch(raw, list(gyro))
    det = task.detector
    dets = det.detect_batch(None, n=n)
    assert sum(len(d) for d in dets) > 0
    grey = task.preview(n=n, width=320, height=200)
    files = task.preview(n=n, width=320, height=200, color=True)
    assert grey == det.preview_jpeg(n=n, width=320, height=200, overlay=True) and task.preview(n=n, width=320, height=200, color=False) == grey
    for i in range(n):
        want = PC.triples_vec(raw[i], "BGRA", sw, sh, 4 * sw, o, 320, 200, [d.corners() for d in dets[i]])
        assert files[i] == EC.encode_ycc(want, 50, 0), i
    det.close()


def test_device_form(built):
    """Raw frames in the caller's device memory at an odd base address, stride and pitch above the minimum; nothing staged."""
    import torch
    W, H, n = 66, 49, 3
    rng = np.random.default_rng(8)
    det = detector(W, H, 2)
    for fourcc, o in [("YUYV", "counterclockwise"), ("BGRA", "rotate-180"), ("RGB3", "none")]:
        sw, sh = R.source_size(W, H, o)
        stride = R.min_stride(fourcc, sw) + 7
        pitch = stride * sh + 13
        raw = [PC.pack_colour(rng, fourcc, sw, sh, stride) for _ in range(n)]
        dev = torch.full((3 + pitch * n,), 0x99, dtype=torch.uint8, device="cuda")
        for i, f in enumerate(raw):
            dev[3 + i * pitch:3 + i * pitch + stride * sh] = torch.from_numpy(f.reshape(-1)).cuda()
        torch.cuda.synchronize()
        ptr = dev.data_ptr() + 3
        assert ptr % 2 == 1
        for width, height in [(0, 0), (37, 21)]:
            pw, ph, _ = EC.layout(width, height, W, H)
            idx = [2, 0]                                         # (n_frames = 3 exceeds nothing: only n is bounded by max_batch)
            tri = det.preview_color_device(ptr, n, stride, pitch, fourcc, o, idx, width=width, height=height)
            files = det.preview_jpeg_color_device(ptr, n, stride, pitch, fourcc, o, idx, width=width, height=height, restart_rows=3)
            for k, f in enumerate(idx):
                want = PC.triples_vec(raw[f], fourcc, sw, sh, stride, o, pw, ph)
                assert np.array_equal(tri[k], want) and files[k] == EC.encode_ycc(want, 50, 3), (fourcc, o, width, k)
        assert rc_of(lambda: det.preview_color_device(ptr, n, stride, pitch, fourcc, o, [3])) == A.CK_EINVAL          # index past n_frames
        assert rc_of(lambda: det.preview_color_device(ptr, n, stride - 8, pitch, fourcc, o, [0])) == A.CK_EINVAL     # stride below the minimum
        assert rc_of(lambda: det.preview_color_device(ptr, n, stride, stride * sh - 1, fourcc, o, [0])) == A.CK_EINVAL
    det.close()


def test_ring_form(built):
    """Two slots of a raw ring: the colour files of slot 0 before and after detect ran on slot 1; other rings are refused."""
    from chalkydri_amd.detector import IngestRing
    W, H = 130, 33
    rng = np.random.default_rng(13)
    det = detector(W, H, 2)
    fourcc, o = "UYVY", "clockwise"
    sw, sh = R.source_size(W, H, o)
    ring = IngestRing(det, 2, fourcc=fourcc, orientation=o)
    raw = [[PC.pack_colour(rng, fourcc, sw, sh) for _ in range(2)] for _ in range(2)]
    for s in (0, 1):
        for i in range(2):
            ring.write(s, i, raw[s][i])
        ring.submit(s, 2)
    want = [[PC.triples_vec(f, fourcc, sw, sh, R.min_stride(fourcc, sw), o, 37, 21) for f in raw[s]] for s in (0, 1)]
    kw = dict(width=37, height=21, restart_rows=1)
    first = ring.preview_jpeg_color(0, [1, 0], **kw)
    assert first == [EC.encode_ycc(want[0][1], 50, 1), EC.encode_ycc(want[0][0], 50, 1)]
    dets1, _ = ring.detect(1, 2)
    assert ring.preview_jpeg_color(0, [1, 0], **kw) == first
    assert np.array_equal(ring.preview_color(1, n=2, **kw), np.stack(want[1]))
    assert ring.preview_jpeg_color(1, n=2, **kw) == [EC.encode_ycc(P, 50, 1) for P in want[1]]
    dets1b, _ = ring.detect(1, 2)                                   # the slot is as it was
    assert [[d.corners().tobytes() for d in fr] for fr in dets1b] == [[d.corners().tobytes() for d in fr] for fr in dets1]
    assert rc_of(lambda: ring.preview_jpeg_color(0, [2], **kw)) == A.CK_EINVAL       # the slot was submitted with 2 frames
    assert rc_of(lambda: ring.preview_jpeg_color(2, n=1, **kw)) == A.CK_EINVAL
    ring.close()
    for other in (IngestRing(det, 1), IngestRing(det, 1, fourcc="MJPG")):
        assert rc_of(lambda: other.preview_jpeg_color(0, n=0)) == A.CK_EUNSUPPORTED
        assert rc_of(lambda: other.preview_color(0, n=0)) == A.CK_EUNSUPPORTED
        other.close()
    grey = IngestRing(det, 1, fourcc="GREY")                         # a raw ring of a luma-first family
    grey.submit(0, 0)
    assert rc_of(lambda: grey.preview_jpeg_color(0, n=0)) == A.CK_EUNSUPPORTED
    grey.close()
    det.close()


def test_truncation_and_device_output(built):
    """cap_per_frame one byte too small for one entry: CK_OK, CK_PREVIEW_TRUNCATED and the true size for it, nothing written past
    its slot, the other files whole; a device `out` gives the same bytes."""
    import torch
    from chalkydri_amd.detector import preview_params
    W, H, n = 64, 48, 3
    rng = np.random.default_rng(17)
    det = detector(W, H, n)
    raw = [PC.pack_colour(rng, "RGBA", W, H) for _ in range(n)]
    raw[1][:] = 77                                                   # a flat frame: the shortest file
    det.upload_raw(raw, "RGBA")
    full = det.preview_jpeg_color(n=n, width=40, height=24)
    lens = [len(b) for b in full]
    cap = max(lens) - 1
    big = lens.index(max(lens))
    assert sum(s > cap for s in lens) == 1
    pp = preview_params(40, 24)
    flat = np.full(n * cap + 1, 0xC3, np.uint8)
    sizes, status = (C.c_int64 * n)(), (C.c_uint32 * n)()
    assert det._L.ck_preview_jpeg_color(det._h, C.byref(pp), None, n, flat.ctypes.data, cap, sizes, status) == A.CK_OK
    assert flat[n * cap] == 0xC3 and list(sizes) == lens
    for i in range(n):
        assert status[i] == (A.CK_PREVIEW_TRUNCATED if i == big else A.CK_PREVIEW_OK)
        used = min(cap, lens[i])
        assert flat[i * cap:i * cap + used].tobytes() == full[i][:used]
        assert np.all(flat[i * cap + used:(i + 1) * cap] == 0xC3)
    dev = torch.full((n * cap + 64,), 0xC3, dtype=torch.uint8, device="cuda")
    sizes2, status2 = (C.c_int64 * n)(), (C.c_uint32 * n)()
    assert det._L.ck_preview_jpeg_color(det._h, C.byref(pp), None, n, C.c_void_p(dev.data_ptr()), cap, sizes2, status2) == A.CK_OK
    torch.cuda.synchronize()
    host = dev.cpu().numpy()
    assert np.array_equal(host[:n * cap], flat[:n * cap]) and np.all(host[n * cap:] == 0xC3)
    assert list(sizes2) == lens and list(status2) == list(status)
    files, sz, st = det.preview_jpeg_color(n=n, width=40, height=24, cap=cap, return_status=True)
    assert sz == lens and [len(b) for b in files] == [min(cap, s) for s in lens] and st == list(status)
    det.close()


def test_refusals_leave_the_handle_working(built):
    """Every refusal of the contract with the call's arguments otherwise valid; after each the handle still encodes."""
    from chalkydri_amd.detector import preview_params, raw_format
    W, H, nb = 64, 48, 2
    rng = np.random.default_rng(19)
    det = detector(W, H, nb)
    L, h = det._L, det._h
    good = preview_params(40, 24)
    _, _, mb = EC.layout(40, 24, W, H)
    out = np.zeros(nb * mb, np.uint8)
    sizes, status = (C.c_int64 * 4)(), (C.c_uint32 * 4)()
    idx = (C.c_int32 * 4)(0, 1, 0, 1)
    raw = [PC.pack_colour(rng, "YUYV", W, H) for _ in range(2)]
    want = PC.triples_vec(raw[0], "YUYV", W, H, 2 * W, "none", 40, 24)

    def jpeg(pp=good, frames=None, n=1, o=out.ctypes.data, cap=mb, s=sizes, hh=h):
        return L.ck_preview_jpeg_color(hh, C.byref(pp) if pp is not None else None, frames, n, o, cap, s, status)

    def tri(pp=good, frames=None, n=1, o=out.ctypes.data, hh=h):
        return L.ck_preview_color(hh, C.byref(pp) if pp is not None else None, frames, n, o)

    def works():
        det.upload_raw(raw, "YUYV")
        return det.preview_jpeg_color([0], width=40, height=24)[0] == want_file(want, 50, 0)
    assert jpeg() == A.CK_EINVAL and tri() == A.CK_EINVAL and jpeg(n=0) == A.CK_EINVAL      # no raw frames staged yet
    assert works()
    assert jpeg(n=2) == A.CK_OK and tri(n=2) == A.CK_OK and jpeg(n=0) == A.CK_OK
    over = preview_params(40, 24, overlay=True)
    assert jpeg(pp=over) == A.CK_EINVAL and tri(pp=over) == A.CK_EINVAL                       # nothing detected on this handle yet
    det.upload(np.zeros((2, H, W), np.uint8))                                                 # staged another way
    assert jpeg() == A.CK_EINVAL and tri() == A.CK_EINVAL and works()
    det.upload_jpeg([E.encode_grey(np.zeros((H, W), np.uint8))])
    assert jpeg() == A.CK_EINVAL and works()
    det.detect_batch(np.zeros((1, H, W), np.uint8))                                           # (a batch call given images stages them)
    assert jpeg() == A.CK_EINVAL and works()
    assert jpeg(pp=over) == A.CK_OK and jpeg(pp=over, n=2) == A.CK_EINVAL                     # that detect call covered frame 0 only
    for fourcc, rows in (("GREY", H), ("NV12", H + H // 2)):
        det.upload_raw([np.zeros((rows, W), np.uint8)], fourcc)
        assert jpeg() == A.CK_EUNSUPPORTED and tri() == A.CK_EUNSUPPORTED, fourcc
        assert len(det.preview_jpeg(n=1)) == 1                                                # the grey preview serves them
        assert works()
    assert jpeg(hh=None) == A.CK_EINVAL and tri(hh=None) == A.CK_EINVAL
    assert jpeg(pp=None) == A.CK_EINVAL and tri(pp=None) == A.CK_EINVAL
    assert jpeg(o=None) == A.CK_EINVAL and tri(o=None) == A.CK_EINVAL
    assert jpeg(s=None) == A.CK_EINVAL and jpeg(cap=0) == A.CK_EINVAL and jpeg(n=-1) == A.CK_EINVAL and tri(n=-1) == A.CK_EINVAL
    assert jpeg(n=3, frames=idx) == A.CK_ECAPACITY and tri(n=3, frames=idx) == A.CK_ECAPACITY
    for bad in ((C.c_int32 * 2)(0, 2), (C.c_int32 * 2)(-1, 0)):
        assert jpeg(n=2, frames=bad) == A.CK_EINVAL and tri(n=2, frames=bad) == A.CK_EINVAL
    for kw in ({"width": 7}, {"height": 7}, {"quality": 0}, {"quality": 101}, {"restart_rows": -1}):
        assert jpeg(pp=preview_params(**kw)) == A.CK_EINVAL, kw
    assert works()
    # the device form's own arguments
    fmt = raw_format("YUYV")
    dev_call = lambda d=out.ctypes.data, f=fmt, nf=1: L.ck_preview_color_device(h, C.byref(good), d, 2 * W, 2 * W * H, C.byref(f) if f else None, None, nf, 0, out.ctypes.data)
    assert dev_call() == A.CK_OK and dev_call(d=None) == A.CK_EINVAL and dev_call(f=None) == A.CK_EINVAL and dev_call(nf=-1) == A.CK_EINVAL
    assert dev_call(f=raw_format("NV12")) == A.CK_EUNSUPPORTED and dev_call(f=A.RawFormat(fmt.fourcc, 4)) == A.CK_EINVAL
    assert works()
    det.close()


def test_stress_helping(built):
    """A small helping of tests/stress_preview_color.py (random geometry, family, orientation, form, quality, restart rows)."""
    import stress_preview_color
    r = stress_preview_color.run(24, 5)
    assert r["mismatching"] == 0, r
