"""The colour preview of MJPEG frames on the GPU (ck_upload_jpeg_color, ck_ingest_create_jpeg_color and the ck_preview_*color*
calls on them).  The expected triples come from tests/np_jpeg_color.py, which tests/test_jpeg_color_host.py ties to
libjpeg-turbo's own YCbCr decode; the expected files are Pillow's.  Every comparison is byte equality."""
import ctypes as C
import io
import os
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg as J  # noqa: E402
import np_jpeg_color as JC  # noqa: E402
import raw_format_ref as R  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLINGS = ("444", "422", "440", "420", "grey")
# stream sizes sw x sh: one MCU at 2x2; ragged MCU columns at 2x1 / 2x2; odd plane width and height (the x == 2cw-1 edge cropped
# away); whole MCUs
STREAMS = [(16, 16), (40, 24), (51, 37), (64, 48)]

_cache = {}


def stream(sw, sh, sampling, dri_rows, seed=0):
    """(bytes, C [sh][sw][3]) of one random stream, made and decoded once: smooth luma + full-range random chroma, restart interval
    none or one MCU row."""
    key = (sw, sh, sampling, dri_rows, seed)
    if key not in _cache:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        yy, xx = np.mgrid[0:sh, 0:sw]
        luma = np.clip(2.5 * xx + 1.5 * yy + rng.normal(0, 25, (sh, sw)) + 20, 0, 255).astype(np.uint8)
        chroma = None if sampling == "grey" else (rng.integers(0, 256, (sh, sw), dtype=np.uint8), rng.integers(0, 256, (sh, sw), dtype=np.uint8))
        b = J.encode(luma, sampling, quality=(85, 60, 95)[seed % 3], restart_interval=dri_rows, restart_rows=bool(dri_rows), chroma=chroma)
        Cc, st = JC.decode_color(b, (sw, sh))
        assert st == J.OK
        _cache[key] = (b, Cc)
    return _cache[key]


def detector(w, h, nb, **kw):
    from chalkydri_amd.detector import AprilTagDetector
    return AprilTagDetector(w, h, max_batch=nb, **kw)


def det_key(dets):
    return [[(d.id(), d.hamming(), d.decision_margin(), d.corners().tobytes(), d.center().tobytes()) for d in f] for f in dets]


def rc_of(call):
    from chalkydri_amd._lib import ChalkydriError
    try:
        call()
    except ChalkydriError as e:
        return e.code
    return A.CK_OK


def check_previews(src, idx, Cs, o, W, H, sizes, dets=None, where=()):
    """src.preview_color / src.preview_jpeg_color of the frames idx (whose triples are Cs[f]) at every (width, height) of sizes:
    the triples equal the reference's and the files equal Pillow's, without restart rows and with one."""
    for width, height in sizes:
        pw, ph = (width or W), (height or H)
        want = [JC.preview_triples(Cs[f], o, pw, ph, None if dets is None else [d.corners() for d in dets[f]]) for f in idx]
        kw = dict(width=width, height=height, overlay=dets is not None)
        got = src.preview_color(idx, **kw)
        assert got.shape == (len(idx), ph, pw, 3)
        for k in range(len(idx)):
            assert np.array_equal(got[k], want[k]), where + (width, height, k, int((got[k] != want[k]).sum()))
        for rr in (0, 1):
            files = src.preview_jpeg_color(idx, quality=50, restart_rows=rr, **kw)
            for k in range(len(idx)):
                assert files[k] == JC.pillow_file(want[k], 50, rr), where + (width, height, rr, k)


@pytest.mark.parametrize("sw,sh", STREAMS)
def test_triples_and_files_equal_libjpeg(built, sw, sh):
    """One stream size x the four orientations (a handle per oriented geometry) x batches of 5 with the five samplings mixed in one
    call (without restart markers, and with one interval per MCU row) and batches of 1: statuses and staged luma equal
    ck_upload_jpeg_oriented's, the triples at identity size equal orient(C), the triples at a reduced size and the files equal the
    reference's, before and after a detect (overlay on: no tag in this content, so the mask is empty and the call must still agree)."""
    for quarter in (False, True):
        W, H = (sh, sw) if quarter else (sw, sh)
        det = detector(W, H, 5)
        small = (16, 24) if quarter else (24, 16)
        small = (min(small[0], W), min(small[1], H))
        for oi, o in enumerate(("clockwise", "counterclockwise") if quarter else ("none", "rotate-180")):
            batches = [[stream(sw, sh, s, dri) for s in SAMPLINGS] for dri in (0, 1)]
            batches.append([stream(sw, sh, SAMPLINGS[(oi + 2 * quarter) % 4], 1, seed=1)])
            batches.append([stream(sw, sh, SAMPLINGS[3 - (oi + 2 * quarter) % 4], 0, seed=2)])
            for bi, batch in enumerate(batches):
                data, Cs = [b for b, _ in batch], [c for _, c in batch]
                n, st = det.upload_jpeg(data, o, return_status=True)
                luma = det.quad_image(None, n).copy()       # (quad_decimate 1, no filter: the quad image is the staged frame)
                n2, st2 = det.upload_jpeg(data, o, return_status=True, color=True)
                assert (n2, st2) == (n, st) and st == [A.CK_JPEG_OK] * n
                assert np.array_equal(det.quad_image(None, n), luma), (o, bi)
                idx = list(range(n))[::-1]
                check_previews(det, idx, Cs, o, W, H, [(0, 0), small], where=(o, bi))
                for f in range(n):
                    assert np.array_equal(luma[f], R.orient_vec(Cs[f][..., 0], o))
                dets = det.detect_batch(None, n=n)
                check_previews(det, idx, Cs, o, W, H, [small], dets=dets, where=(o, bi, "overlay"))
                check_previews(det, idx[:1], Cs, o, W, H, [small], where=(o, bi, "after detect"))
        det.close()


def scene_jpeg(frame, o, subsampling, seed, quality=90):
    """A JPEG whose oriented luma is close to the rendered tag scene `frame`, with colour around it; and its triples C."""
    rgb = R.source_of(R.grey_to_rgb(frame, seed), o)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb), "RGB").save(buf, "JPEG", quality=quality, subsampling=subsampling)
    b = buf.getvalue()
    return b, JC.pillow_ycc(b)     # (libjpeg's own decode: the restatement equals it, tests/test_jpeg_color_host.py)


def test_overlay_on_a_tag_scene(built):
    """A 640 x 480 tag scene as a 4:2:0 JPEG, mounted clockwise: tags are found, and the overlay's triple lies on exactly the
    reference's pixels at 24 x 16 and at 320 x 240; the files equal Pillow's."""
    from chalkydri_amd import scenes
    W, H = 640, 480
    frame = scenes.bench_stream(7, 1, W, H, 4)[0][0]
    o = "clockwise"
    b, Cc = scene_jpeg(frame, o, 2, 1)
    assert Cc.shape == (W, H, 3) and (Cc[..., 1] != 128).any()
    det = detector(W, H, 1)
    det.upload_jpeg([b], o, color=True)
    dets = det.detect_batch(None, n=1)
    assert len(dets[0]) > 0
    check_previews(det, [0], [Cc], o, W, H, [(24, 16), (320, 240)], dets=dets)
    P = det.preview_color([0], width=320, height=240, overlay=True)[0]
    Q = det.preview_color([0], width=320, height=240)[0]
    changed = (P != Q).any(axis=-1)
    assert changed.sum() > 20 and (P[changed] == np.array([150, 44, 21], np.uint8)).all()
    det.close()


def test_failed_frames_are_grey_black(built):
    """A truncated, a progressive (SOF2) and a wrong-geometry stream among good ones: (0, 128, 128) with their status bits, the
    neighbours exact, the call CK_OK — under no turn and under a quarter turn."""
    sw, sh = 40, 24
    good = [stream(sw, sh, "420", 0), stream(sw, sh, "444", 1), stream(sw, sh, "grey", 0)]
    g0 = good[0][0]
    sof = g0.index(b"\xff\xc0")
    progressive = g0[:sof + 1] + b"\xc2" + g0[sof + 2:]
    batch = [good[0][0], g0[:len(g0) // 2], good[1][0], progressive, stream(sh, sw, "420", 0)[0], good[2][0]]
    bad = np.zeros((sh, sw, 3), np.uint8)
    bad[..., 1:] = 128
    Cs = [good[0][1], bad, good[1][1], bad, bad, good[2][1]]
    for Cc, b in zip(Cs, batch):      # the restatement's own rules give the same frames
        assert np.array_equal(JC.decode_color(b, (sw, sh))[0], Cc)
    for o in ("none", "counterclockwise"):
        W, H = R.source_size(sw, sh, o)   # (the map is its own inverse on sizes)
        det = detector(W, H, len(batch))
        n, st = det.upload_jpeg(batch, o, return_status=True, color=True)
        assert st == [0, A.CK_JPEG_CORRUPT, 0, A.CK_JPEG_UNSUPPORTED, A.CK_JPEG_GEOMETRY, 0]
        check_previews(det, list(range(n)), Cs, o, W, H, [(0, 0), (16, 16)], where=(o,))
        det.close()


def test_ring_keeps_a_slots_colours(built):
    """ck_ingest_create_jpeg_color with 2 slots: slot 0's colours are still there after slot 1 was submitted, a resubmitted slot 0
    has the new ones, statuses come through, and the detections through the ring equal the plain path's."""
    from chalkydri_amd import scenes
    from chalkydri_amd.detector import IngestRing
    W, H = 640, 480
    o = "rotate-180"
    frames = scenes.bench_stream(11, 6, W, H, 4)[0]
    sets = [[scene_jpeg(frames[2 * k + i], o, (2, 1, 0)[(k + i) % 3], 3 * k + i) for i in range(2)] for k in range(3)]
    det = detector(W, H, 2)
    ring = IngestRing(det, 2, fourcc="MJPG", orientation=o, color=True)
    for slot in (0, 1):
        for i, (b, _) in enumerate(sets[slot]):
            ring.write(slot, i, b)
        ring.submit(slot, 2)
    assert ring.jpeg_status(0, 2) == [0, 0] and ring.jpeg_status(1, 2) == [0, 0]
    check_previews(_Slot(ring, 0), [1, 0], [c for _, c in sets[0]], o, W, H, [(0, 0), (24, 16)], where=("slot 0",))
    check_previews(_Slot(ring, 1), [0, 1], [c for _, c in sets[1]], o, W, H, [(24, 16)], where=("slot 1",))
    got = {slot: ring.detect(slot, 2)[0] for slot in (1, 0)}   # (slot 0 last: the overlay draws the last call's detections)
    check_previews(_Slot(ring, 0), [0, 1], [c for _, c in sets[0]], o, W, H, [(64, 48)], dets=got[0], where=("slot 0 overlay",))
    for i, (b, _) in enumerate(sets[2]):
        ring.write(0, i, b)
    ring.submit(0, 2)
    check_previews(_Slot(ring, 0), [0, 1], [c for _, c in sets[2]], o, W, H, [(24, 16)], where=("slot 0 again",))
    check_previews(_Slot(ring, 1), [1], [c for _, c in sets[1]], o, W, H, [(24, 16)], where=("slot 1 still",))
    ring.detect(0, 2)
    ring.close()
    for k in (0, 1):
        det.upload_jpeg([b for b, _ in sets[k]], o)
        want = det.detect_batch(None, n=2)
        assert det_key(want) == det_key(got[k]) and sum(len(f) for f in want) > 0
    det.close()


class _Slot:
    """A ring slot with the detector's preview signature."""

    def __init__(self, ring, slot):
        self.ring, self.slot = ring, slot

    def preview_color(self, idx, **kw):
        return self.ring.preview_color(self.slot, idx, **kw)

    def preview_jpeg_color(self, idx, **kw):
        return self.ring.preview_jpeg_color(self.slot, idx, **kw)


def test_refusals_are_unchanged(built):
    """What the colour preview refused before it still refuses with the same code; the new state ends with the next staging."""
    from chalkydri_amd.detector import IngestRing
    sw, sh = 40, 24
    b, Cc = stream(sw, sh, "420", 0)
    det = detector(sw, sh, 2)
    call = lambda: det.preview_jpeg_color([0], width=0, height=0)  # noqa: E731
    assert rc_of(call) == A.CK_EINVAL                               # nothing staged
    det.upload_jpeg([b])
    assert rc_of(call) == A.CK_EINVAL                               # a plain ck_upload_jpeg
    det.upload_jpeg([b], color=True)
    assert rc_of(call) == A.CK_OK
    assert rc_of(lambda: det.preview_color([1], width=0, height=0)) == A.CK_EINVAL   # an index past the frames of that call
    det.upload([np.ascontiguousarray(Cc[..., 0])])
    assert rc_of(call) == A.CK_EINVAL                               # ck_upload_frames ends it
    det.upload_jpeg([b], color=True)
    det.decode_jpeg([b])
    assert rc_of(call) == A.CK_EINVAL                               # ... and so does a luma-only decode
    det.upload_raw([np.ascontiguousarray(Cc[..., 0])], "GREY")
    assert rc_of(call) == A.CK_EUNSUPPORTED                         # a luma-first raw upload
    st = (C.c_uint32 * 4)()
    from chalkydri_amd.detector import _jpeg_frames
    arr, keep = _jpeg_frames([b, b, b])
    assert det._L.ck_upload_jpeg_color(det._h, arr, 3, 0, st) == A.CK_ECAPACITY
    assert det._L.ck_upload_jpeg_color(det._h, arr, 1, 7, st) == A.CK_EINVAL
    assert det._L.ck_upload_jpeg_color(det._h, None, 1, 0, st) == A.CK_EINVAL
    assert det._L.ck_upload_jpeg_color(det._h, arr, 0, 0, st) == A.CK_OK
    assert rc_of(lambda: det.preview_color([0], width=0, height=0)) == A.CK_EINVAL   # no frame of that call
    ring = IngestRing(det, 2, fourcc="MJPG", max_frame_bytes=1 << 16)   # (noise chroma: larger than the default bound sw * sh)
    ring.write(0, 0, b)
    ring.submit(0, 1)
    assert rc_of(lambda: ring.preview_jpeg_color(0, [0], width=0, height=0)) == A.CK_EUNSUPPORTED
    assert rc_of(lambda: ring.preview_color(0, [0], width=0, height=0)) == A.CK_EUNSUPPORTED
    ring.detect(0, 1)
    ring.close()
    g = C.c_void_p()
    assert det._L.ck_ingest_create_jpeg_color(det._h, 2, 5, 0, C.byref(g)) == A.CK_EINVAL
    assert det._L.ck_ingest_create_jpeg_color(det._h, 9, 0, 0, C.byref(g)) == A.CK_EINVAL
    with pytest.raises(ValueError):
        IngestRing(det, 2, fourcc="YUYV", color=True)
    det.close()


def test_workspace_grows_between_calls(built):
    """A 4:2:0 call of one frame, then a 4:4:4 call of four on the same handle (more coefficients, larger planes): exact bytes."""
    sw, sh = 64, 48
    det = detector(sw, sh, 4)
    first = [stream(sw, sh, "420", 0)]
    det.upload_jpeg([b for b, _ in first], color=True)
    check_previews(det, [0], [c for _, c in first], "none", sw, sh, [(0, 0)])
    second = [stream(sw, sh, "444", dri, seed) for dri, seed in ((0, 0), (1, 0), (0, 3), (1, 4))]
    det.upload_jpeg([b for b, _ in second], color=True)
    check_previews(det, [3, 2, 1, 0], [c for _, c in second], "none", sw, sh, [(0, 0), (24, 16)])
    det.close()


def test_apriltags_task_previews_mjpeg_in_colour(built):
    """AprilTags(..., fourcc="MJPG", jpeg_color=True).preview(color=True) gives the colour file of the processed frame; without
    the keyword the call is refused as before."""
    from chalkydri_amd import scenes
    from chalkydri_amd.apriltags import AprilTags
    W, H = 640, 480
    frames, gyro, layout, calib, r2c = scenes.bench_stream(3, 1, W, H, 4)
    b, Cc = scene_jpeg(frames[0], "none", 2, 5)
    task = AprilTags(W, H, layout, calib, r2c, fourcc="MJPG", jpeg_color=True)
    task.process_raw_batch([b], list(gyro))
    f = task.preview(n=1, overlay=False, color=True, width=160, height=120)[0]
    assert f == JC.pillow_file(JC.preview_triples(Cc, "none", 160, 120), 50, 0)
    task.detector.close()
    plain = AprilTags(W, H, layout, calib, r2c, fourcc="MJPG")
    plain.process_raw_batch([b], list(gyro))
    assert rc_of(lambda: plain.preview(n=1, overlay=False, color=True)) == A.CK_EINVAL
    plain.detector.close()
