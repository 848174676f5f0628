"""Baseline JPEG decode on the GPU (ck_upload_jpeg / ck_jpeg_luma_batch): the device's luma bit-identical to the numpy restatement
of libjpeg (tests/np_jpeg.py) and, where Pillow is importable, to libjpeg itself; per-frame failures; the detector path after a
JPEG upload identical to the one after a raw upload."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg as J  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLINGS = ["444", "422", "440", "420", "grey"]
RESTARTS = [(0, False), (1, False), (1, True), (7, False)]   # none, 1 MCU, one MCU row, 7 MCUs
QUALITIES = [30, 85, 100]


def textured(rng, h, w, noise=False):
    if noise:
        return (rng.random((h, w)) * 256).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 60 * np.sin(xx / 23.0 + rng.random() * 6) * np.cos(yy / 31.0) + 40 * ((xx // 37 + yy // 29) % 2)
    return np.clip(base + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)


def detector(w, h, nb):
    from chalkydri_amd.detector import AprilTagDetector
    return AprilTagDetector(w, h, max_batch=nb)


def check_batch(det, streams):
    got, st = det.decode_jpeg(streams, return_status=True)
    for i, b in enumerate(streams):
        want, wst = J.decode_luma(b)
        assert wst == J.OK and st[i] == A.CK_JPEG_OK, (i, st[i], wst)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
    return got


@pytest.mark.parametrize("w,h", [(16, 16), (40, 24)])
def test_full_matrix_small(built, w, h):
    """Every sampling x restart interval x quality (noise at q100: long codes, large coefficients), one batch per size."""
    rng = np.random.default_rng(w * 1000 + h)
    streams = []
    for samp in SAMPLINGS:
        for ri, rows in RESTARTS:
            for q in QUALITIES:
                streams.append(J.encode(textured(rng, h, w, noise=q == 100), sampling=samp, quality=q, restart_interval=ri, restart_rows=rows))
    det = detector(w, h, len(streams))
    check_batch(det, streams)
    det.close()


@pytest.mark.parametrize("w,h", [(1280, 800), (1600, 1304), (1283, 797)])
def test_large_frames(built, w, h):
    """The reference cameras' sizes and a ragged one: every sampling and every restart kind, qualities cycled, one batch that
    mixes samplings, tables (standard, shuffled, absent) and quantisation precision."""
    rng = np.random.default_rng(w + h)
    streams = []
    for k, samp in enumerate(SAMPLINGS):
        ri, rows = RESTARTS[k % 4]
        kw = dict(sampling=samp, quality=QUALITIES[k % 3], restart_interval=ri, restart_rows=rows)
        if k == 1:
            kw["tables"] = {(1, 0): J.shuffled_table(1, 0, rng), (0, 1): J.shuffled_table(0, 1, rng)}
        if k == 2:
            kw["dht"] = False
        if k == 3:
            kw["q16"] = True
        streams.append(J.encode(textured(rng, h, w), **kw))
    # q100 on noise: long codes, large coefficients, thousands of subsequences per frame
    streams.append(J.encode(textured(rng, h, w, noise=True), sampling="444", quality=100))
    det = detector(w, h, len(streams))
    check_batch(det, streams)
    det.close()


def test_pillow_streams_match_libjpeg(built):
    PIL = pytest.importorskip("PIL.Image")
    w, h = 1280, 800
    rng = np.random.default_rng(11)
    streams = []
    for k, kw in enumerate([dict(quality=85, subsampling=2), dict(quality=95, subsampling=0, optimize=True),
                            dict(quality=60, subsampling=1, restart_marker_rows=1), dict(quality=90, subsampling=2, restart_marker_blocks=3)]):
        rgb = np.stack([textured(rng, h, w), textured(rng, h, w), textured(rng, h, w)], -1)
        buf = io.BytesIO()
        PIL.fromarray(rgb).save(buf, "JPEG", **kw)
        streams.append(buf.getvalue())
    det = detector(w, h, len(streams))
    got = check_batch(det, streams)
    for i, b in enumerate(streams):
        im = PIL.open(io.BytesIO(b))
        im.draft("L", im.size)
        assert np.array_equal(got[i], np.asarray(im.convert("L"))), i
    det.close()


def splice_corrupt(b):
    """The stream with FF 00 FF 00 (sixteen 1-bits after unstuffing) spliced into its scan at the first place where the numpy
    decoder then reports corruption."""
    P = J.parse(b)
    for frac in (0.5, 0.3, 0.7, 0.2, 0.8, 0.1, 0.9):
        at = P["scan_off"] + int((len(b) - P["scan_off"] - 2) * frac)
        if b[at - 1] == 0xFF:
            at += 1
        c = b[:at] + b"\xff\x00\xff\x00" + b[at:]
        if J.decode_luma(c)[1] == J.CORRUPT:
            return c
    raise AssertionError("no corrupting splice found")


def rst_positions(b):
    """Offsets of the RSTn markers in the stream (0xFF followed by 0xD0..0xD7 only occurs as a marker in a scan)."""
    off = J.parse(b)["scan_off"]
    return [i for i in range(off, len(b) - 1) if b[i] == 0xFF and 0xD0 <= b[i + 1] <= 0xD7]


def test_mixed_batch_flags_bad_frames(built):
    w, h = 320, 240
    rng = np.random.default_rng(3)
    good = [J.encode(textured(rng, h, w), sampling=s, quality=80, restart_interval=ri) for s, ri in (("420", 0), ("444", 5), ("grey", 0))]
    # DCs far outside the sample range: the device must wrap them through the masked range-limit table as libjpeg does
    extreme = J.encode(textured(rng, h, w), sampling="444", quality=1, dc_offset=np.arange(-300, 300, 7))
    want_extreme = J.decode_luma(extreme)[0]
    assert ((want_extreme != 0) & (want_extreme != 255)).any() and (want_extreme == 0).any() and (want_extreme == 255).any()
    base = J.encode(textured(rng, h, w), sampling="420", quality=90)
    segs = [(base[i + 1], i) for i in range(2, len(base) - 1) if base[i] == 0xFF and base[i + 1] == 0xC0]
    progressive = base[:segs[0][1] + 1] + b"\xc2" + base[segs[0][1] + 2:]
    wrong_size = J.encode(textured(rng, h - 8, w), sampling="420")
    truncated = base[:len(base) // 2]
    assert J.decode_luma(truncated)[1] == J.CORRUPT
    spliced = splice_corrupt(base)
    # restart markers: one missing, one out of sequence, one in excess (after the last interval)
    dri = J.encode(textured(rng, h, w), sampling="420", quality=85, restart_interval=4)
    rp = rst_positions(dri)
    assert len(rp) > 3
    rst_missing = dri[:rp[2]] + dri[rp[2] + 2:]
    rst_order = dri[:rp[2] + 1] + bytes([0xD0 + ((dri[rp[2] + 1] - 0xD0 + 3) & 7)]) + dri[rp[2] + 2:]
    nxt = 0xD0 + ((dri[rp[-1] + 1] - 0xD0 + 1) & 7)
    rst_excess = dri[:-2] + bytes([0xFF, nxt]) + dri[-2:]
    for bad in (rst_missing, rst_order, rst_excess):
        assert J.decode_luma(bad)[1] == J.CORRUPT
    batch = [good[0], progressive, good[1], wrong_size, truncated, good[2], spliced, extreme, rst_missing, rst_order, rst_excess, dri]
    det = detector(w, h, len(batch))
    out, st = det.decode_jpeg(batch, return_status=True)
    C_ = A.CK_JPEG_CORRUPT
    assert st == [0, A.CK_JPEG_UNSUPPORTED, 0, A.CK_JPEG_GEOMETRY, C_, 0, C_, 0, C_, C_, C_, 0]
    for i, b in ((0, good[0]), (2, good[1]), (5, good[2]), (7, extreme), (11, dri)):
        assert np.array_equal(out[i], J.decode_luma(b)[0]), i
    for i in (1, 3, 4, 6, 8, 9, 10):
        assert not out[i].any(), i
    # upload_jpeg reports the same bits
    n, st2 = det.upload_jpeg(batch, return_status=True)
    assert n == len(batch) and st2 == st
    det.close()


def test_argument_errors(built):
    from chalkydri_amd.detector import _bind, _jpeg_frames
    from chalkydri_amd._lib import lib
    L = _bind(lib())
    w, h = 64, 48
    det = detector(w, h, 2)
    b = J.encode(textured(np.random.default_rng(0), h, w))
    arr, keep = _jpeg_frames([b, b, b])
    out = np.zeros((3, h, w), np.uint8)
    st = (C.c_uint32 * 3)()
    assert L.ck_upload_jpeg(None, arr, 1, st) == A.CK_EINVAL
    assert L.ck_upload_jpeg(det._h, None, 1, st) == A.CK_EINVAL
    assert L.ck_upload_jpeg(det._h, arr, -1, st) == A.CK_EINVAL
    assert L.ck_upload_jpeg(det._h, arr, 3, st) == A.CK_ECAPACITY
    assert L.ck_jpeg_luma_batch(det._h, arr, 1, None, st) == A.CK_EINVAL
    assert L.ck_jpeg_luma_batch(det._h, arr, 3, out.ctypes.data, st) == A.CK_ECAPACITY
    short = (A.JpegFrame * 1)()
    short[0].data, short[0].size = keep[0].ctypes.data, 3
    assert L.ck_upload_jpeg(det._h, short, 1, st) == A.CK_EINVAL
    short[0].data, short[0].size = None, 100
    assert L.ck_upload_jpeg(det._h, short, 1, st) == A.CK_EINVAL
    assert L.ck_upload_jpeg(det._h, arr, 0, None) == A.CK_OK
    assert L.ck_jpeg_luma_batch(det._h, arr, 2, out.ctypes.data, None) == A.CK_OK   # status may be NULL
    assert np.array_equal(out[0], J.decode_luma(b)[0])
    det.close()


def scene_streams(n, w, h):
    from chalkydri_amd import scenes
    frames, gyro, layout, calib, r2c = scenes.bench_stream(2, n, w, h, 6)
    return frames, gyro, layout, calib, r2c, [J.encode(f, sampling="420", quality=90) for f in frames]


def test_end_to_end_matches_raw_upload(built):
    """upload_jpeg -> detect / process / last_tag_poses gives byte-identical records to upload(numpy-decoded luma) -> the same."""
    from chalkydri_amd.apriltags import AprilTags
    from chalkydri_amd.detector import tag_pose_params
    w, h, n = 640, 480, 4
    frames, gyro, layout, calib, r2c, streams = scene_streams(n, w, h)
    decoded = np.stack([J.decode_luma(b)[0] for b in streams])
    task = AprilTags(w, h, layout, calib, r2c, cam_id=1, max_batch=n)
    det = task.detector
    c = calib["OpenCVModel5"]
    pp = tag_pose_params(c["fx"], c["fy"], c["cx"], c["cy"])

    def run(upload):
        upload()
        dets = det.detect_batch(None, n=n)
        poses = det.last_tag_poses(pp, raw=True)
        upload()
        recs, valid = task.process_batch(None, list(gyro), n=n)
        key = [[(d.id(), d.hamming(), d.decision_margin(), d.corners().tobytes(), d.center().tobytes()) for d in f] for f in dets]
        return key, [[bytes(p) for p in f] for f in poses], bytes(recs), valid.tolist()
    a = run(lambda: det.upload_jpeg(streams))
    b = run(lambda: det.upload(decoded))
    assert a == b
    assert sum(len(f) for f in a[0]) > 0


def test_scene_truth_ids_found(built):
    from chalkydri_amd import scenes
    w, h = 1280, 800
    lay = scenes.wall_layout(6, cols=3)
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
    streams, truths = [], []
    for i, pose in enumerate([(1.0, 0.0, 0.0), (1.3, 0.2, 0.05), (0.8, -0.2, -0.05)]):
        frame, truth = scenes.render_view(100 + i, w, h, w * 0.9, lay, pose, r2c)
        streams.append(J.encode(frame, sampling="420", quality=90))
        truths.append({t["id"] for t in truth["tags"]})
    det = detector(w, h, len(streams))
    assert det.upload_jpeg(streams) == len(streams)
    dets = det.detect_batch(None, n=len(streams))
    for f, want in zip(dets, truths):
        assert want and want <= {d.id() for d in f}, (want, [d.id() for d in f])
    det.close()


def test_stress_script_runs_clean(built):
    """tests/stress_jpeg.py (randomised streams against the numpy restatement) in a child, a short run: no mismatch."""
    import json
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "stress_jpeg.py"), "25", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mismatching"] == 0 and res["frames"] > 25
