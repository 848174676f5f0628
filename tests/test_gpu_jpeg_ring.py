"""MJPEG frames turned by the camera's mounting, through the synchronous upload and through the JPEG ingest ring (DESIGN.md §4c,
"JPEG frames: orientation and the ring").  The streams come from tests/np_jpeg.py: encode, the expected bytes from np_jpeg.decode_luma
+ tests/raw_format_ref.py: orient (and from libjpeg itself where Pillow imports); every comparison is byte equality."""
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg as J  # noqa: E402
import raw_format_ref as R  # noqa: E402
import scenes  # noqa: E402
from test_gpu_jpeg import textured  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

try:
    from PIL import Image
except Exception:  # pragma: no cover
    Image = None

pytestmark = pytest.mark.gpu

SAMPLINGS = ["grey", "444", "422", "440", "420"]
SIZES = [(640, 480), (272, 200), (641, 479), (100, 75), (1280, 800), (24, 1000)]   # ORIENTED width x height
R2C = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}


def libjpeg_luma(b):
    im = Image.open(io.BytesIO(b))
    im.draft("L", im.size)
    return np.asarray(im.convert("L"))


def det_key(dets):
    return [[(d.id(), d.hamming(), d.decision_margin(), d.corners().tobytes(), d.center().tobytes()) for d in f] for f in dets]


@pytest.mark.parametrize("W,H", SIZES)
def test_oriented_decode(built, W, H):
    """4 orientations x 5 samplings x DRI / none x DHT / none at one oriented size: decode_jpeg(orientation) and the frames
    upload_jpeg stages equal orient(libjpeg's luma).  Sizes with sw % 8, sh % 8 != 0 put partial MCUs on both sides of the turn."""
    from chalkydri_amd.detector import AprilTagDetector
    rng = np.random.default_rng(W * 7 + H)
    cases = [(s, dri, dht) for s in SAMPLINGS for dri in (0, 5) for dht in (True, False)]
    det = AprilTagDetector(W, H, max_batch=len(cases))
    for quarter in (False, True):
        sw, sh = (H, W) if quarter else (W, H)
        streams = [J.encode(textured(rng, sh, sw), sampling=s, quality=(85, 60, 95)[k % 3], restart_interval=dri, dht=dht)
                   for k, (s, dri, dht) in enumerate(cases)]
        S = []
        for b, case in zip(streams, cases):
            luma, st = J.decode_luma(b)
            assert st == J.OK and luma.shape == (sh, sw), case
            if Image is not None:
                assert np.array_equal(luma, libjpeg_luma(b)), case
            S.append(luma)
        for o in (("clockwise", "counterclockwise") if quarter else ("none", "rotate-180")):
            want = np.stack([R.orient_vec(s, o) for s in S])
            got, st = det.decode_jpeg(streams, return_status=True, orientation=o)
            assert st == [A.CK_JPEG_OK] * len(cases), (o, st)
            for i, case in enumerate(cases):
                assert np.array_equal(got[i], want[i]), (o, case, int((got[i] != want[i]).sum()))
            n, st = det.upload_jpeg(streams, o, return_status=True)
            assert n == len(cases) and st == [A.CK_JPEG_OK] * n
            staged = det.quad_image(None, n)      # (quad_decimate 1, no filter: the quad image is the staged frame)
            assert np.array_equal(staged, want), o
    det.close()


def test_orientation_none_is_ck_upload_jpeg(built):
    """The new entry points at CK_ORIENT_NONE against the old ones on a batch with good and bad streams: pixels and status words."""
    from chalkydri_amd.detector import AprilTagDetector, _jpeg_frames
    w, h = 323, 241
    rng = np.random.default_rng(5)
    good = [J.encode(textured(rng, h, w), sampling=s, quality=80, restart_interval=ri) for s, ri in (("420", 0), ("422", 3), ("grey", 0))]
    sof = good[0].index(b"\xff\xc0")
    progressive = good[0][:sof + 1] + b"\xc2" + good[0][sof + 2:]
    batch = [good[0], progressive, good[1], J.encode(textured(rng, h - 8, w)), good[0][:len(good[0]) // 2], good[2]]
    n = len(batch)
    det = AprilTagDetector(w, h, max_batch=n)
    arr, keep = _jpeg_frames(batch)
    old, new = np.zeros((n, h, w), np.uint8), np.ones((n, h, w), np.uint8)
    st_old, st_new, st_up_old, st_up_new = ((C.c_uint32 * n)() for _ in range(4))
    assert det._L.ck_jpeg_luma_batch(det._h, arr, n, old.ctypes.data, st_old) == A.CK_OK
    assert det._L.ck_jpeg_luma_batch_oriented(det._h, arr, n, A.CK_ORIENT_NONE, new.ctypes.data, st_new) == A.CK_OK
    assert np.array_equal(old, new) and list(st_old) == list(st_new)
    assert list(st_old) == [0, A.CK_JPEG_UNSUPPORTED, 0, A.CK_JPEG_GEOMETRY, A.CK_JPEG_CORRUPT, 0]
    assert det._L.ck_upload_jpeg(det._h, arr, n, st_up_old) == A.CK_OK
    a = det.quad_image(None, n)
    assert det._L.ck_upload_jpeg_oriented(det._h, arr, n, A.CK_ORIENT_NONE, st_up_new) == A.CK_OK
    b = det.quad_image(None, n)
    assert np.array_equal(a, b) and np.array_equal(a, old) and list(st_up_old) == list(st_up_new) == list(st_old)
    # on a handle: orientation outside 0..3, and the capacity
    assert det._L.ck_upload_jpeg_oriented(det._h, arr, n, 4, st_up_new) == A.CK_EINVAL
    assert det._L.ck_upload_jpeg_oriented(det._h, arr, n, -1, st_up_new) == A.CK_EINVAL
    arr7, keep7 = _jpeg_frames(batch + [good[0]])
    assert det._L.ck_upload_jpeg_oriented(det._h, arr7, n + 1, 0, None) == A.CK_ECAPACITY
    det.close()


def test_unturned_stream_on_a_quarter_turn_handle(built):
    """A W x H stream where the mounting needs H x W is CK_JPEG_GEOMETRY and staged as zeros; its neighbours are right."""
    from chalkydri_amd.detector import AprilTagDetector
    W, H = 200, 120
    rng = np.random.default_rng(9)
    right = [J.encode(textured(rng, W, H), sampling=s) for s in ("420", "444")]     # H wide, W tall
    wrong = J.encode(textured(rng, H, W), sampling="420")                           # W wide, H tall
    det = AprilTagDetector(W, H, max_batch=3)
    for o in ("clockwise", "counterclockwise"):
        got, st = det.decode_jpeg([right[0], wrong, right[1]], return_status=True, orientation=o)
        assert st == [0, A.CK_JPEG_GEOMETRY, 0]
        assert not got[1].any()
        for i, b in ((0, right[0]), (2, right[1])):
            assert np.array_equal(got[i], R.orient_vec(J.decode_luma(b)[0], o)), (o, i)
    # and the other way round: the turned stream on an unturned handle
    got, st = det.decode_jpeg([wrong, right[0]], return_status=True, orientation="rotate-180")
    assert st == [0, A.CK_JPEG_GEOMETRY] and not got[1].any()
    assert np.array_equal(got[0], R.orient_vec(J.decode_luma(wrong)[0], "rotate-180"))
    det.close()


def scene_batches(W, H, o, n, batches, seed=700):
    """`batches` lists of n streams whose ORIENTED frames are W x H views of a tag wall, and the gyro headings."""
    layout = scenes.wall_layout(6, cols=3)
    calib = scenes.pinhole_calib(W * 0.95, W / 2.0, H / 2.0)
    rng = np.random.default_rng(seed)
    out, gyros = [], []
    for b in range(batches):
        streams, g = [], []
        for i in range(n):
            pose = (rng.uniform(1.6, 2.6), rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1))
            fr, _ = scenes.render_view(seed + 10 * b + i, W, H, W * 0.95, layout, pose, R2C, noise_amp=2)
            streams.append(J.encode(R.source_of(fr, o), sampling=("420", "422", "grey")[(b + i) % 3], quality=90, restart_interval=(0, 6)[i % 2]))
            g.append(pose[2])
        out.append(streams); gyros.append(g)
    return layout, calib, out, gyros


@pytest.mark.parametrize("o", R.ORIENTATIONS)
def test_ring_equals_upload_path(built, o):
    """Detections and 64-byte records from a JPEG ring byte-equal to upload_jpeg + detect_uploaded / process_uploaded on the same
    handle: two slots submitted before either is processed, processed in the opposite order, each slot reused three times with
    other frames (and other counts)."""
    from chalkydri_amd.apriltags import AprilTags
    from chalkydri_amd.detector import IngestRing
    W, H, n = 480, 360, 3
    layout, calib, batches, gyros = scene_batches(W, H, o, n, 6)
    task = AprilTags(W, H, layout, calib, R2C, cam_id=3, max_batch=n)
    det = task.detector
    ring = IngestRing(det, 2, fourcc="MJPG", orientation=o, max_frame_bytes=max(len(b) for s in batches for b in s))
    assert ring.stride == 0 and not det._L.ck_ingest_frame(ring._g, 0, 0)

    def reference(streams, g):
        k = det.upload_jpeg(streams, o)
        dets = det_key(det.detect_batch(None, n=k))
        det.upload_jpeg(streams, o)
        recs, valid = task.process_batch(None, g, n=k)
        return dets, [bytes(r) for r in recs], valid.tolist()

    total = 0
    for rnd in range(3):
        k = (n, n - 1, 1)[rnd]                                     # the count changes from one use of a slot to the next
        pair = [(batches[2 * rnd + s][:k], gyros[2 * rnd + s][:k]) for s in range(2)]
        want = [reference(*p) for p in pair]
        for s in range(2):
            for i, b in enumerate(pair[s][0]):
                ring.write(s, i, b)
            ring.submit(s, k)                                      # both in flight before either is processed
        for s in (1, 0):                                           # the opposite order
            recs, valid = ring.process(s, k, task._pp, pair[s][1], np.ones(k, np.uint8))
            dets, status = ring.detect(s, k)
            assert ring.jpeg_status(s, k) == [0] * k
            assert (det_key(dets), [bytes(r) for r in recs], valid.astype(bool).tolist()) == want[s], (o, rnd, s)
            total += sum(len(f) for f in dets)
    assert total >= 2 * (n + n - 1 + 1)                             # the wall's tags are found: the equality is not one of empty lists
    ring.close()
    det.close()


def test_ring_status_words_and_bad_frames(built):
    """A slot that mixes good, truncated-scan, wrong-geometry and progressive frames: ck_ingest_jpeg_status equals ck_upload_jpeg's
    words, the bad frames yield no detections, the good ones theirs."""
    from chalkydri_amd.detector import AprilTagDetector, IngestRing
    W, H = 480, 360
    o = "clockwise"
    layout, calib, batches, _ = scene_batches(W, H, o, 2, 1, seed=900)
    good = batches[0]
    sof = good[0].index(b"\xff\xc0")
    progressive = good[0][:sof + 1] + b"\xc2" + good[0][sof + 2:]
    truncated = good[1][:len(good[1]) // 2]
    assert J.decode_luma(truncated)[1] == J.CORRUPT
    unturned = J.encode(textured(np.random.default_rng(1), H, W))   # W x H where H x W is due
    batch = [good[0], truncated, unturned, progressive, good[1], b"\xff\xd8\xff\xd9"]
    n = len(batch)
    det = AprilTagDetector(W, H, max_batch=n)
    k, want_st = det.upload_jpeg(batch, o, return_status=True)
    want = det_key(det.detect_batch(None, n=n))
    assert want_st == [0, A.CK_JPEG_CORRUPT, A.CK_JPEG_GEOMETRY, A.CK_JPEG_UNSUPPORTED, 0, A.CK_JPEG_CORRUPT]
    ring = IngestRing(det, 1, fourcc="JPEG", orientation=o)        # max_frame_bytes 0 = sw * sh
    for i, b in enumerate(batch):
        ring.write(0, i, b)
    ring.submit(0, n)
    assert ring.jpeg_status(0, n) == want_st
    dets, _ = ring.detect(0, n)
    assert det_key(dets) == want
    assert [len(f) for f in dets][1:4] == [0, 0, 0] and len(dets[5]) == 0 and len(dets[0]) > 0 and len(dets[4]) > 0
    ring.close()
    det.close()


def test_ring_misuse(built):
    """Every refusal the header names, each followed by a valid call that succeeds."""
    from chalkydri_amd.detector import AprilTagDetector, IngestRing, fourcc
    W, H, n = 160, 120, 2
    rng = np.random.default_rng(2)
    b = J.encode(textured(rng, H, W), sampling="420")
    det = AprilTagDetector(W, H, max_batch=n)
    L = det._L
    buf = np.frombuffer(b, np.uint8)
    cap = len(b) + 10
    ring = IngestRing(det, 2, fourcc="MJPG", max_frame_bytes=cap)
    g = ring._g
    st = (C.c_uint32 * n)()

    def write(slot, index, data=buf, size=None):
        return L.ck_ingest_write_jpeg(g, slot, index, data.ctypes.data, data.size if size is None else size)
    # submit with an unwritten index
    assert write(0, 0) == A.CK_OK
    assert L.ck_ingest_submit(g, 0, 2) == A.CK_EINVAL
    assert write(0, 1) == A.CK_OK and L.ck_ingest_submit(g, 0, 2) == A.CK_OK
    assert L.ck_ingest_jpeg_status(g, 0, 2, st) == A.CK_OK and list(st) == [0, 0]
    # ... "written since the slot's last submit": the frames of the last submit do not count
    assert L.ck_ingest_submit(g, 0, 1) == A.CK_EINVAL
    assert write(0, 0) == A.CK_OK and L.ck_ingest_submit(g, 0, 1) == A.CK_OK
    # size > max_frame_bytes
    big = np.concatenate([buf, np.zeros(cap + 1 - buf.size, np.uint8)])
    assert write(1, 0, big) == A.CK_ECAPACITY
    fits = np.concatenate([buf, np.zeros(cap - buf.size, np.uint8)])   # (trailing bytes after EOI are ignored)
    assert write(1, 0, fits) == A.CK_OK
    # null data, size < 4, slot and index out of range
    assert L.ck_ingest_write_jpeg(g, 1, 0, None, 100) == A.CK_EINVAL
    assert write(1, 0, size=3) == A.CK_EINVAL
    for slot, index in ((2, 0), (-1, 0), (0, n), (0, -1)):
        assert write(slot, index) == A.CK_EINVAL, (slot, index)
    assert L.ck_ingest_submit(g, 2, 1) == A.CK_EINVAL
    assert L.ck_ingest_jpeg_status(g, 2, 1, st) == A.CK_EINVAL
    # n > max_batch
    assert L.ck_ingest_submit(g, 1, n + 1) == A.CK_EINVAL
    assert L.ck_ingest_submit(g, 1, 1) == A.CK_OK
    assert L.ck_ingest_jpeg_status(g, 1, 2, st) == A.CK_EINVAL           # not the count the slot was submitted with
    assert L.ck_ingest_jpeg_status(g, 1, 1, st) == A.CK_OK and st[0] == 0
    # the raw entry points on a JPEG ring
    img = (A.ImageU8 * 1)()
    frame = textured(rng, H, W)
    img[0].buf, img[0].width, img[0].height, img[0].stride = frame.ctypes.data, W, H, W
    assert L.ck_ingest_write(g, 0, 0, img, fourcc("GREY")) == A.CK_EUNSUPPORTED
    assert not L.ck_ingest_frame(g, 0, 0) and L.ck_ingest_stride(g) == 0
    want = J.decode_luma(b)[0]
    assert np.array_equal(det.decode_jpeg([b])[0], want)
    # ck_ingest_write_jpeg / ck_ingest_jpeg_status on a luma ring and on a raw ring
    for kw in ({}, {"fourcc": "YUYV"}):
        other = IngestRing(det, 1, **kw)
        assert L.ck_ingest_write_jpeg(other._g, 0, 0, buf.ctypes.data, buf.size) == A.CK_EINVAL
        assert L.ck_ingest_jpeg_status(other._g, 0, 0, st) == A.CK_EINVAL
        if not kw:
            other.write(0, 0, frame)
            other.submit(0, 1)
            assert len(other.detect(0, 1)[0]) == 1
        other.close()
    # creation
    gg = C.c_void_p()
    assert L.ck_ingest_create_jpeg(det._h, 2, 4, 0, C.byref(gg)) == A.CK_EINVAL
    assert L.ck_ingest_create_jpeg(det._h, 2, 0, -5, C.byref(gg)) == A.CK_EINVAL
    assert L.ck_ingest_create_jpeg(det._h, 9, 0, 0, C.byref(gg)) == A.CK_EINVAL
    assert L.ck_ingest_create_jpeg(det._h, 1, 3, 0, C.byref(gg)) == A.CK_OK
    L.ck_ingest_destroy(gg)
    # the ring still works after all of it
    assert write(0, 0) == A.CK_OK and L.ck_ingest_submit(g, 0, 1) == A.CK_OK
    dets, _ = ring.detect(0, 1)
    assert ring.jpeg_status(0, 1) == [0] and len(dets) == 1
    ring.close()
    det.close()


def test_task_layer_takes_mjpg(built):
    """AprilTags(fourcc="MJPG", orientation="clockwise").process_raw(streams) equals process_batch on the decoded, turned luma."""
    from chalkydri_amd.apriltags import AprilTags
    W, H, n = 480, 640, 3
    o = "clockwise"
    layout, calib, batches, gyros = scene_batches(W, H, o, n, 1, seed=1100)
    streams = batches[0]
    want_luma = np.stack([R.orient_vec(J.decode_luma(b)[0], o) for b in streams])
    assert want_luma.shape == (n, H, W)
    task = AprilTags(W, H, layout, calib, R2C, cam_id=4, max_batch=n, fourcc="MJPG", orientation=o)
    recs, valid = task.process_raw(streams, gyros[0])
    got = [bytes(r) for r in recs]
    assert np.array_equal(task.detector.quad_image(None, n), want_luma)
    plain = AprilTags(W, H, layout, calib, R2C, cam_id=4, max_batch=n)
    recs2, valid2 = plain.process_batch(want_luma, gyros[0])
    assert got == [bytes(r) for r in recs2] and valid.tolist() == valid2.tolist() and valid.all()
    task.detector.close()
    plain.detector.close()


def test_stress_script_runs_clean(built):
    """tests/stress_jpeg_ring.py (random sizes, orientations, streams and slot counts) in a child, a short run: no mismatch."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "stress_jpeg_ring.py"), "12", "7"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mismatching"] == 0 and res["frames"] >= 12
