"""The planar 4:2:0 raw formats with their chroma planes on the GPU (NV12, NV21, I420, YV12 with CK_RAW_PLANES).
The colour preview's triples and files and the blob detector's pixels, planes and records equal tests/raw_planes_ref.py, and equal,
byte for byte, what the YUYV path that was there before returns for the frame's YUYV twin — through the handle's raw staging, a
caller's device memory and a raw ingest ring; the staged luma and everything detected from it are those of the upload without the
flag; the refusals of the contract; determinism.

Handles 17 x 19 (both odd: the last chroma row and column serve one pixel), 34 x 18 (not square under the quarter turns) and
64 x 48; n = 3 with frames [2, 0, 2]; strides at the minimum, + 2 and + 16."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_blobs as NB  # noqa: E402
import np_jpeg_enc_color as EC  # noqa: E402
import raw_format_ref as R  # noqa: E402
import raw_planes_ref as P  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

HANDLES = [(17, 19), (34, 18), (64, 48)]
EXTRA = (0, 2, 16)
IDX = [2, 0, 2]
PREVIEWS = [(0, 0), (8, 8), (24, 16)]


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


def want_file(Pic, q, rr):
    key = (Pic.shape, Pic.tobytes(), q, rr)
    if key not in _files:
        _files[key] = EC.encode_ycc(Pic, q, rr)
    return _files[key]


def frames_of(planes, code, stride, seed=0):
    """One frame per (y, cb, cr) of `planes`, random bytes wherever no plane holds a sample."""
    return [P.pack_planes(y, cb, cr, code, stride, pad_byte=None, seed=seed + k) for k, (y, cb, cr) in enumerate(planes)]


def device_frames(torch, raw, pitch, base, fill=0x99):
    dev = torch.full((base + pitch * len(raw) + 1,), fill, dtype=torch.uint8, device="cuda")
    for i, f in enumerate(raw):
        dev[base + i * pitch:base + i * pitch + f.size] = torch.from_numpy(f.reshape(-1)).cuda()
    torch.cuda.synchronize()
    return dev


@pytest.mark.parametrize("W,H", HANDLES)
def test_triples_files_and_the_twin(built, W, H):
    """Four fourccs x four turns x three strides: preview_color at the identity size, 8 x 8 and 24 x 16 equals the restatement and
    the scale rule, preview_jpeg_color at quality 50 with restart rows 0 and 1 equals its encoding, and both equal what the YUYV
    path returns for the YUYV twin.  The samples are the same for every fourcc and stride of a turn, so is every expected byte."""
    rng = np.random.default_rng(W * 100 + H)
    det = detector(W, H, 3)
    bad = []
    for o in R.ORIENTATIONS:
        sw, sh = R.source_size(W, H, o)
        planes = [P.random_planes(rng, sw, sh) for _ in range(3)]
        ref = frames_of(planes, "NV12", P.min_stride(sw))
        O = [P.triples_vec(f, "NV12", sw, sh, P.min_stride(sw), o) for f in ref]
        # the twin, through the 4:2:2 source kind
        twins = [P.yuyv_twin(f, "NV12", sw, sh, P.min_stride(sw)) for f in ref]
        det.upload_raw(twins, "YUYV", o)
        twin = {}
        for width, height in PREVIEWS:
            twin[width, height] = (det.preview_color(IDX, width=width, height=height),
                                   [det.preview_jpeg_color(IDX, width=width, height=height, quality=50, restart_rows=rr) for rr in (0, 1)])
        for code in P.FOURCCS:
            for e in EXTRA:
                stride = P.min_stride(sw) + e
                raw = frames_of(planes, code, stride, seed=e)
                det.upload_raw(raw, code, o, planes=True)
                for width, height in PREVIEWS:
                    pw, ph, _ = EC.layout(width, height, W, H)
                    want = [P.preview(O[f], pw, ph) for f in IDX]
                    got = det.preview_color(IDX, width=width, height=height)
                    assert got.shape == (3, ph, pw, 3)
                    ok = np.array_equal(got, np.stack(want)) and np.array_equal(got, twin[width, height][0])
                    for rr in (0, 1):
                        files = det.preview_jpeg_color(IDX, width=width, height=height, quality=50, restart_rows=rr)
                        ok = ok and files == [want_file(p, 50, rr) for p in want] and files == twin[width, height][1][rr]
                    if not ok:
                        bad.append((code, o, stride, width, height))
    det.close()
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("W,H", HANDLES)
def test_luma_is_the_flagless_uploads(built, W, H):
    """The staged luma after a planes=True upload equals the flag-less upload's of the same bytes and the restatement of §4d; two
    uploads that differ only in the bytes no plane holds give the same luma and the same triples."""
    rng = np.random.default_rng(W + H)
    det = detector(W, H, 3)
    for code in P.FOURCCS:
        for o in R.ORIENTATIONS:
            sw, sh = R.source_size(W, H, o)
            planes = [P.random_planes(rng, sw, sh) for _ in range(3)]
            for e in EXTRA:
                stride = P.min_stride(sw) + e
                raw = frames_of(planes, code, stride, seed=1)
                with_flag = det.raw_luma(raw, code, o, planes=True)
                tri = det.preview_color(IDX, width=0, height=0)
                assert np.array_equal(det.quad_image(None, n=3), with_flag)
                assert np.array_equal(with_flag, det.raw_luma(raw, code, o)), (code, o, stride)
                for k in range(3):
                    assert np.array_equal(with_flag[k], R.orient_vec(planes[k][0], o)), (code, o, stride, k)
                other = frames_of(planes, code, stride, seed=77)
                assert e == 0 or any((a != b).any() for a, b in zip(raw, other))       # (a stride above the minimum has padding)
                assert np.array_equal(det.raw_luma(other, code, o, planes=True), with_flag)
                assert np.array_equal(det.preview_color(IDX, width=0, height=0), tri)
    det.close()


def test_tag_scene_detect_process_overlay_and_task(built):
    """A 640 x 480 tag scene as the luma of NV12 / YV12 frames: detections and process records after a planes=True upload equal
    the flag-less upload's, the overlay lies on the restatement's pixels, and the task layer serves preview(color=True) and blobs."""
    from chalkydri_amd import blobs as B, scenes
    from chalkydri_amd.apriltags import AprilTags
    W, H, n = 640, 480, 2
    frames, gyro, layout, calib, r2c = scenes.bench_stream(1, n, W, H, 4)
    rng = np.random.default_rng(5)
    keys = lambda dets: [[(d.id(), d.corners().tobytes()) for d in fr] for fr in dets]
    for code, o, e in (("NV12", "none", 0), ("YV12", "clockwise", 16)):
        sw, sh = R.source_size(W, H, o)
        stride = P.min_stride(sw) + e
        planes = []
        for f in frames:
            _, cb, cr = P.random_planes(rng, sw, sh)
            planes.append((R.source_of(f, o), cb, cr))
        raw = frames_of(planes, code, stride)
        plain = AprilTags(W, H, layout, calib, r2c, cam_id=1, max_batch=n, fourcc=code, orientation=o)
        rec0, valid0 = plain.process_raw_batch(raw, list(gyro))
        dets0 = plain.detector.detect_batch(None, n=n)
        assert sum(len(d) for d in dets0) > 0
        assert rc_of(lambda: plain.preview(n=n, color=True)) == A.CK_EUNSUPPORTED          # without the flag: as before
        plain.detector.close()
        classes = [B.ColorClass(h_min=100, h_max=140, s_min=60, v_min=60, min_area=9)]
        task = AprilTags(W, H, layout, calib, r2c, cam_id=1, max_batch=n, fourcc=code, orientation=o, planes=True, blobs=classes)
        rec1, valid1 = task.process_raw_batch(raw, list(gyro))
        assert [bytes(r) for r in rec1] == [bytes(r) for r in rec0] and list(valid1) == list(valid0)
        det = task.detector
        dets1 = det.detect_batch(None, n=n)
        assert keys(dets1) == keys(dets0)
        rgb = det.blob_rgb(n=n)
        got = task.blobs
        want = B.blobs_host(task._blob_params, rgb)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        files = task.preview(n=n, width=320, height=200, color=True)
        for i in range(n):
            O = P.triples_vec(raw[i], code, sw, sh, stride, o)
            assert np.array_equal(rgb[i], NB.ycc_rgb(O))
            corners = [d.corners() for d in dets1[i]]
            wantP = P.preview(O, 320, 200, corners)
            assert (wantP != P.preview(O, 320, 200)).any()                                   # the overlay is there
            assert np.array_equal(det.preview_color([i], width=320, height=200, overlay=True)[0], wantP)
            assert files[i] == EC.encode_ycc(wantP, 50, 0), i
        det.close()
    with pytest.raises(ValueError):
        AprilTags(W, H, layout, calib, r2c, fourcc="YUYV", planes=True)


def blob_scene(rng, sw, sh):
    """Saturated rectangles drawn in YCbCr: the luma at full resolution with edges on odd coordinates, the chroma at chroma
    resolution, on a grey, noisy background; two of them touch the last row and column."""
    cw, ch = P.chroma_size(sw, sh)
    y = rng.integers(20, 60, (sh, sw)).astype(np.uint8)
    cb = rng.integers(120, 128, (ch, cw)).astype(np.uint8)
    cr = rng.integers(128, 136, (ch, cw)).astype(np.uint8)
    orange, blue = (150, 40, 220), (90, 230, 100)
    rects = [(1, 1, sw // 3 | 1, sh // 3 | 1, orange), (sw // 2 | 1, 3, sw, sh // 2 | 1, blue), (3, sh // 2 | 1, sw // 2 - 1 | 1, sh, orange)]
    for x0, y0, x1, y1, (Y, CB, CR) in rects:
        y[y0:y1, x0:x1] = Y
        cb[y0 >> 1:(y1 + 1) >> 1, x0 >> 1:(x1 + 1) >> 1] = CB
        cr[y0 >> 1:(y1 + 1) >> 1, x0 >> 1:(x1 + 1) >> 1] = CR
    return y, cb, cr


@pytest.mark.parametrize("W,H", HANDLES)
def test_blobs(built, W, H):
    """blob_rgb equals ycc_rgb of the restatement's triples; detect_blobs and blob_mask (both stages) equal the host twin's bytes on
    those pixels, and equal the records and planes of the YUYV twin through the 4:2:2 source kind."""
    from chalkydri_amd import blobs as B
    rng = np.random.default_rng(W * 3 + H)
    det = detector(W, H, 3)
    pp = B.blob_params([B.ColorClass(h_min=0, h_max=25, s_min=100, v_min=100, min_area=4),
                        B.ColorClass(h_min=95, h_max=135, s_min=100, v_min=60, min_area=4)], erode=1, dilate=1)
    some = 0
    for o in R.ORIENTATIONS:
        sw, sh = R.source_size(W, H, o)
        planes = [blob_scene(rng, sw, sh) for _ in range(3)]
        ref = frames_of(planes, "NV12", P.min_stride(sw))
        rgb = np.stack([NB.ycc_rgb(P.triples_vec(ref[f], "NV12", sw, sh, P.min_stride(sw), o)) for f in IDX])
        want = B.blobs_host(pp, rgb)
        masks = {(c, s): B.mask_host(pp, rgb, c, s) for c in (0, 1) for s in (0, 1)}
        some += int(want[1].sum())
        det.upload_raw([P.yuyv_twin(f, "NV12", sw, sh, P.min_stride(sw)) for f in ref], "YUYV", o)
        twin = det.detect_blobs(pp, IDX)
        twin_masks = {k: det.blob_mask(pp, k[0], k[1], IDX) for k in masks}
        for code in P.FOURCCS:
            for e in EXTRA:
                stride = P.min_stride(sw) + e
                det.upload_raw(frames_of(planes, code, stride, seed=e), code, o, planes=True)
                assert np.array_equal(det.blob_rgb(IDX), rgb), (code, o, stride)
                got = det.detect_blobs(pp, IDX)
                for g, w, t, name in zip(got, want, twin, ("records", "counts", "status")):
                    assert g.tobytes() == w.tobytes() == t.tobytes(), (name, code, o, stride)
                for k, m in masks.items():
                    gm = det.blob_mask(pp, k[0], k[1], IDX)
                    assert gm.tobytes() == m.tobytes() == twin_masks[k].tobytes(), (k, code, o, stride)
    det.close()
    assert some > 0


@pytest.mark.parametrize("W,H", HANDLES)
def test_device_form(built, W, H):
    """Frames in the caller's device memory: the base one byte off (two for I420 / YV12), a stride above the minimum and a pitch
    above stride * (sh + ch) — a plane offset taken from the pitch or from the minimum stride would read the wrong bytes.  Every
    device call equals the host-upload form."""
    import torch
    from chalkydri_amd import blobs as B
    rng = np.random.default_rng(W * 5 + H)
    det = detector(W, H, 3)
    host = detector(W, H, 3)
    pp = B.blob_params([B.ColorClass(h_min=0, h_max=25, s_min=100, v_min=100, min_area=4)], erode=1, dilate=1)
    for code in P.FOURCCS:
        for o in R.ORIENTATIONS:
            sw, sh = R.source_size(W, H, o)
            cw, ch = P.chroma_size(sw, sh)
            stride = P.min_stride(sw) + 6
            pitch = stride * (sh + ch) + 11
            base = 2 if code in ("I420", "YV12") else 1
            raw = frames_of([blob_scene(rng, sw, sh) for _ in range(3)], code, stride)
            dev = device_frames(torch, raw, pitch, base)
            ptr = dev.data_ptr() + base
            host.upload_raw(raw, code, o, planes=True)
            O = [P.triples_vec(f, code, sw, sh, stride, o) for f in raw]
            for width, height in ((0, 0), (8, 8)):
                tri = det.preview_color_device(ptr, 3, stride, pitch, code, o, IDX, width=width, height=height, planes=True)
                assert np.array_equal(tri, host.preview_color(IDX, width=width, height=height)), (code, o, width)
                pw, ph, _ = EC.layout(width, height, W, H)
                assert np.array_equal(tri, np.stack([P.preview(O[f], pw, ph) for f in IDX]))
                files = det.preview_jpeg_color_device(ptr, 3, stride, pitch, code, o, IDX, width=width, height=height, restart_rows=1, planes=True)
                assert files == host.preview_jpeg_color(IDX, width=width, height=height, restart_rows=1), (code, o, width)
            src = (ptr, 3, stride, pitch, code, o, True)
            assert np.array_equal(det.blob_rgb(IDX, device=src), host.blob_rgb(IDX))
            assert np.array_equal(det.blob_mask(pp, 0, 1, IDX, device=src), host.blob_mask(pp, 0, 1, IDX))
            got, want = det.detect_blobs_device(pp, ptr, 3, stride, pitch, code, o, frames=IDX, planes=True), host.detect_blobs(pp, IDX)
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes(), (code, o)
            assert det.blob_time(pp, ptr, 3, stride, pitch, code, o, reps=1, planes=True) > 0
            det.upload_raw_device(ptr, 3, stride, pitch, code, o, planes=True)
            assert np.array_equal(det.quad_image(None, n=3), host.quad_image(None, n=3))
            # the pitch must hold the chroma rows; the stride the chroma pairs
            short = stride * (sh + ch) - 1
            assert rc_of(lambda: det.preview_color_device(ptr, 3, stride, short, code, o, [0], planes=True)) == A.CK_EINVAL
            assert rc_of(lambda: det.upload_raw_device(ptr, 3, stride, short, code, o, planes=True)) == A.CK_EINVAL
            assert rc_of(lambda: det.detect_blobs_device(pp, ptr, 3, stride, short, code, o, frames=[0], planes=True)) == A.CK_EINVAL
            assert rc_of(lambda: det.preview_color_device(ptr, 3, stride, pitch, code, o, [0])) == A.CK_EUNSUPPORTED      # without the flag
            del dev
    det.close()
    host.close()


def test_ring_form(built):
    """A planes=True ring of two slots, written from caller frames of a larger stride: detect equals the flag-less ring's; colour
    and blobs of slot 0 are still right after slot 1 was submitted; another layout's fourcc is refused."""
    from chalkydri_amd import blobs as B
    from chalkydri_amd.detector import IngestRing
    W, H = 34, 18
    rng = np.random.default_rng(21)
    det = detector(W, H, 2)
    pp = B.blob_params([B.ColorClass(h_min=0, h_max=25, s_min=100, v_min=100, min_area=4)], erode=1, dilate=1)
    keys = lambda dets: [[(d.id(), d.corners().tobytes()) for d in fr] for fr in dets]
    for code, o in (("NV12", "clockwise"), ("I420", "none"), ("YV12", "counterclockwise"), ("NV21", "rotate-180")):
        sw, sh = R.source_size(W, H, o)
        cw, ch = P.chroma_size(sw, sh)
        stride = P.min_stride(sw) + 10
        ring = IngestRing(det, 2, fourcc=code, orientation=o, planes=True)
        plain = IngestRing(det, 2, fourcc=code, orientation=o)
        assert ring.slot_view(0).shape == (2, sh + ch, ring.stride) and ring.stride == (P.min_stride(sw) + 15) // 16 * 16
        assert plain.slot_view(0).shape[1] == sh
        raw = [frames_of([blob_scene(rng, sw, sh) for _ in range(2)], code, stride, seed=s) for s in (0, 1)]
        for s in (0, 1):
            for i in range(2):
                ring.write(s, i, raw[s][i])
                plain.write(s, i, raw[s][i])
        ring.submit(0, 2)
        plain.submit(0, 2)
        O = [[P.triples_vec(f, code, sw, sh, stride, o) for f in raw[s]] for s in (0, 1)]
        first = ring.preview_color(0, [1, 0], width=0, height=0)
        assert np.array_equal(first, np.stack([O[0][1], O[0][0]])), (code, o)
        ring.submit(1, 2)
        plain.submit(1, 2)
        d1, st1 = ring.detect(1, 2)
        d0, st0 = plain.detect(1, 2)
        assert keys(d1) == keys(d0) and np.array_equal(st1, st0)
        assert np.array_equal(ring.preview_color(0, [1, 0], width=0, height=0), first)
        assert ring.preview_jpeg_color(0, [0], width=0, height=0, restart_rows=1) == [want_file(O[0][0], 50, 1)]
        rgb = np.stack([NB.ycc_rgb(O[0][1]), NB.ycc_rgb(O[0][0])])
        for g, w in zip(ring.detect_blobs(0, pp, [1, 0]), B.blobs_host(pp, rgb)):
            assert g.tobytes() == w.tobytes(), (code, o)
        assert np.array_equal(ring.preview_color(1, n=2, width=8, height=8), np.stack([P.preview(p, 8, 8) for p in O[1]]))
        stats = ring.exposure_stats(1, n=2)
        assert np.array_equal(stats["luma"], plain.exposure_stats(1, n=2)["luma"])
        # with the flag the four fourccs are four families; without it they are one, as before
        for other in P.FOURCCS:
            want_rc = A.CK_OK if other == code else A.CK_EUNSUPPORTED
            assert rc_of(lambda: ring.write(1, 0, raw[1][0], other)) == want_rc, (code, other)
            assert rc_of(lambda: plain.write(1, 0, raw[1][0], other)) == A.CK_OK
        assert rc_of(lambda: ring.write(1, 0, raw[1][0], "GREY")) == A.CK_EUNSUPPORTED
        assert rc_of(lambda: ring.write(1, 0, np.ascontiguousarray(raw[1][0][:, :P.min_stride(sw) - 2]))) == A.CK_EINVAL
        assert rc_of(lambda: plain.preview_color(0, n=1)) == A.CK_EUNSUPPORTED
        ring.close()
        plain.close()
    det.close()


def test_refusals_leave_the_handle_working(built):
    from chalkydri_amd.detector import IngestRing
    W, H = 17, 19
    rng = np.random.default_rng(31)
    det = detector(W, H, 2)
    planes = [P.random_planes(rng, W, H) for _ in range(2)]
    good = frames_of(planes, "NV12", 18)
    want = np.stack([P.triples_vec(f, "NV12", W, H, 18, "none") for f in good])

    def works():
        det.upload_raw(good, "NV12", planes=True)
        return np.array_equal(det.preview_color(n=2, width=0, height=0), want)
    assert works()
    # a stride equal to sw for an odd sw: one byte short of the last chroma pair
    rows = H + (H + 1) // 2
    assert rc_of(lambda: det.upload_raw([np.zeros((rows, 17), np.uint8)], "NV12", planes=True)) == A.CK_EINVAL and works()
    assert rc_of(lambda: det.upload_raw([np.zeros((rows, 17), np.uint8)], "NV12")) == A.CK_OK and works()                # (fine without the flag)
    # an odd stride with two half-stride planes
    for code in ("I420", "YV12"):
        assert rc_of(lambda: det.upload_raw([np.zeros((rows, 19), np.uint8)], code, planes=True)) == A.CK_EINVAL and works()
        assert rc_of(lambda: det.upload_raw([np.zeros((rows, 20), np.uint8)], code, planes=True)) == A.CK_OK
        assert rc_of(lambda: det.raw_luma([np.zeros((rows, 19), np.uint8)], code, planes=True)) == A.CK_EINVAL and works()
    assert rc_of(lambda: det.upload_raw([np.zeros((rows, 19), np.uint8)], "NV21", planes=True)) == A.CK_OK and works()
    # the flag with a fourcc that has no chroma planes
    for code, cols in (("GREY", 17), ("YUYV", 36)):
        assert rc_of(lambda: det.upload_raw([np.zeros((rows, cols), np.uint8)], code, planes=True)) == A.CK_EUNSUPPORTED and works()
        assert rc_of(lambda: IngestRing(det, 1, fourcc=code, planes=True)) == A.CK_EUNSUPPORTED and works()
        assert rc_of(lambda: det.preview_color_device(1, 1, 64, 64 * rows, code, "none", [0], planes=True)) == A.CK_EUNSUPPORTED
    # a bit outside 0x103
    assert rc_of(lambda: det.upload_raw(good, "NV12", 0x200 | A.CK_RAW_PLANES)) == A.CK_EINVAL and works()
    assert rc_of(lambda: det.upload_raw(good, "NV12", 4, planes=True)) == A.CK_EINVAL and works()
    # after a planes=True upload, a flag-less upload of the same fourcc takes the colour away again
    det.upload_raw(good, "NV12")
    assert rc_of(lambda: det.preview_color(n=2)) == A.CK_EUNSUPPORTED and rc_of(lambda: det.blob_rgb(n=2)) == A.CK_EUNSUPPORTED
    assert rc_of(lambda: det.preview_jpeg_color(n=2)) == A.CK_EUNSUPPORTED
    assert len(det.preview_jpeg(n=2)) == 2 and works()
    # ... and frames staged another way make it CK_EINVAL, the rule of the raw staging
    det.upload(np.zeros((2, H, W), np.uint8))
    assert rc_of(lambda: det.preview_color(n=2)) == A.CK_EINVAL and works()
    assert rc_of(lambda: det.preview_color([2])) == A.CK_EINVAL and works()
    det.close()


def test_two_calls_return_the_same_bytes(built):
    from chalkydri_amd import blobs as B
    W, H = 64, 48
    rng = np.random.default_rng(41)
    det = detector(W, H, 3)
    pp = B.blob_params([B.ColorClass(h_min=0, h_max=25, s_min=100, v_min=100, min_area=4)], erode=1, dilate=1)
    for code, o in (("NV21", "clockwise"), ("I420", "rotate-180")):
        sw, sh = R.source_size(W, H, o)
        raw = frames_of([blob_scene(rng, sw, sh) for _ in range(3)], code, P.min_stride(sw) + 2)
        runs = []
        for _ in range(2):
            det.upload_raw(raw, code, o, planes=True)
            rec = det.detect_blobs(pp, IDX)
            runs.append((det.preview_color(IDX, width=24, height=16).tobytes(), det.preview_jpeg_color(IDX, width=0, height=0, restart_rows=1),
                         det.blob_rgb(IDX).tobytes(), rec[0].tobytes(), rec[1].tobytes(), det.blob_mask(pp, 0, 0, IDX).tobytes()))
        assert runs[0] == runs[1], (code, o)
    det.close()
