"""Coloured game pieces on the GPU (ck_detect_blobs*, ck_blob_rgb*, ck_blob_mask*): the RGB the classifier sees
equals the colour preview's reference triples through the numpy ycc-to-rgb (or the source's own bytes), the planes equal the host
twin's at both stages, and the records equal ck_blobs_host's byte for byte — from the handle's raw staging, a caller's device
memory, a raw ring and the JPEG colour form; patterns laid across the word and row seams of the run labelling; the capacity rule;
determinism; and that a blob call leaves the detector's own state alone."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_blobs as NB  # noqa: E402
import preview_color_ref as PC  # noqa: E402
import raw_format_ref as R  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "blobs_demo")
ORIENTATIONS = ("none", "clockwise", "rotate-180", "counterclockwise")
ORANGE = dict(h_min=0, h_max=20, s_min=100, v_min=100)


@pytest.fixture(scope="module")
def B(built):
    from chalkydri_amd import blobs
    return blobs


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


def want_rgb(buf, fourcc, sw, sh, stride, o):
    """The oriented RGB the classifier sees of one raw frame."""
    if fourcc in PC.YUV422:
        W, H = R.source_size(sw, sh, o)   # (the turn of a turn's size: the oriented frame's)
        return NB.ycc_rgb(PC.triples_vec(buf, fourcc, sw, sh, stride, o, W, H))
    bpp, ri, gi, bi = R.RGB_ORDER[fourcc]
    b = np.asarray(buf, np.uint8).reshape(-1)
    ms = R.min_stride(fourcc, sw)
    rows = np.lib.stride_tricks.as_strided(b[:(sh - 1) * stride + ms], (sh, ms), (stride, 1))
    px = rows[:, :bpp * sw].reshape(sh, sw, bpp)
    S = np.stack([px[:, :, ri], px[:, :, gi], px[:, :, bi]], -1)
    return np.ascontiguousarray((S, np.rot90(S, -1), S[::-1, ::-1], np.rot90(S, 1))[R.ORIENT_CODE[o]])


def raw_of(picture, fourcc="RGB3", o="none"):
    """The raw frame (minimum stride) of a packed RGB family whose oriented picture is `picture` [H][W][3]."""
    S = np.ascontiguousarray((picture, np.rot90(picture, 1), picture[::-1, ::-1], np.rot90(picture, -1))[R.ORIENT_CODE[o]])
    bpp, ri, gi, bi = R.RGB_ORDER[fourcc]
    out = np.full(S.shape[:2] + (bpp,), 0xEE, np.uint8)
    out[:, :, ri], out[:, :, gi], out[:, :, bi] = S[:, :, 0], S[:, :, 1], S[:, :, 2]
    return out.reshape(S.shape[0], S.shape[1] * bpp)


def paint(mask, on=(255, 40, 0), off=(10, 10, 10)):
    rgb = np.empty(mask.shape + (3,), np.uint8)
    rgb[...] = off
    rgb[mask] = on
    return rgb


def same(got, want, what=()):
    for g, w, name in zip(got, want, ("records", "counts", "status")):
        assert g.tobytes() == w.tobytes(), (name,) + tuple(what)


# ---- device RGB --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(66, 49), (33, 17)])
def test_rgb_equals_the_reference(B, W, H):
    """Every packed family x four orientations, n = 3 with a repeated index; 33 x 17 makes every source width odd (the 4:2:2 pair rule)."""
    rng = np.random.default_rng(W)
    det = detector(W, H, 3)
    for fourcc in PC.FAMILIES:
        for o in ORIENTATIONS:
            sw, sh = R.source_size(W, H, o)
            raw = [PC.pack_colour(rng, fourcc, sw, sh) for _ in range(2)]
            det.upload_raw(raw, fourcc, o)
            got = det.blob_rgb([1, 0, 1])
            for k, f in enumerate((1, 0, 1)):
                assert np.array_equal(got[k], want_rgb(raw[f], fourcc, sw, sh, R.min_stride(fourcc, sw), o)), (fourcc, o, k)
    det.close()


def device_frames(torch, raw, stride, pitch, sh, fill=0x99):
    dev = torch.full((3 + pitch * len(raw),), fill, dtype=torch.uint8, device="cuda")
    for i, f in enumerate(raw):
        dev[3 + i * pitch:3 + i * pitch + stride * sh] = torch.from_numpy(f.reshape(-1)).cuda()
    torch.cuda.synchronize()
    return dev


def test_rgb_padded_stride_and_refusals(B):
    """Caller's device memory at an odd address, a stride above the minimum with a poisoned pad; the colour preview's refusals."""
    import torch
    W, H, n = 50, 37, 2
    det = detector(W, H, 3)
    rng = np.random.default_rng(3)
    for fourcc, o in (("YUYV", "clockwise"), ("BGRA", "rotate-180"), ("RGB3", "counterclockwise")):
        sw, sh = R.source_size(W, H, o)
        stride = R.min_stride(fourcc, sw) + 13
        pitch = stride * sh + 5
        raw = [PC.pack_colour(rng, fourcc, sw, sh, stride, pad_byte=0xFF) for _ in range(n)]
        dev = device_frames(torch, raw, stride, pitch, sh)
        src = (dev.data_ptr() + 3, n, stride, pitch, fourcc, o)
        got = det.blob_rgb([1, 1, 0], device=src)
        for k, f in enumerate((1, 1, 0)):
            assert np.array_equal(got[k], want_rgb(raw[f], fourcc, sw, sh, stride, o)), (fourcc, o, k)
        pp = B.blob_params()
        assert rc_of(lambda: det.detect_blobs_device(pp, *src, frames=[2])) == A.CK_EINVAL                   # index past n_frames
        assert rc_of(lambda: det.detect_blobs_device(pp, src[0], n, stride - 20, pitch, fourcc, o, frames=[0])) == A.CK_EINVAL
        assert rc_of(lambda: det.detect_blobs_device(pp, src[0], n, stride, stride * sh - 1, fourcc, o, frames=[0])) == A.CK_EINVAL
        assert rc_of(lambda: det.detect_blobs_device(pp, *src, frames=[0, 0, 0, 0])) == A.CK_ECAPACITY       # n > max_batch
        assert rc_of(lambda: det.detect_blobs_device(pp, src[0], n, stride, pitch, "NV12", o, frames=[0])) == A.CK_EUNSUPPORTED
        pp.erode = 5
        assert rc_of(lambda: det.detect_blobs_device(pp, *src, frames=[0])) == A.CK_EINVAL
    assert rc_of(lambda: det.blob_rgb([0])) == A.CK_EINVAL     # nothing staged from a colour source
    det.close()


def test_jpeg_colour_form(B):
    """The frames of upload_jpeg(color=True): the decoded triples through ycc-to-rgb; the records equal the twin's."""
    import np_jpeg as J
    import np_jpeg_color as JC
    sw, sh, o = 51, 37, "clockwise"
    W, H = R.source_size(sw, sh, "counterclockwise")
    rng = np.random.default_rng(zlib.crc32(b"blobs"))
    yy, xx = np.mgrid[0:sh, 0:sw]
    luma = np.clip(2.5 * xx + 1.5 * yy + rng.normal(0, 25, (sh, sw)) + 20, 0, 255).astype(np.uint8)
    blocks = lambda: np.kron(rng.integers(0, 256, ((sh + 7) // 8, (sw + 7) // 8)), np.ones((8, 8), int))[:sh, :sw].astype(np.uint8)
    data = J.encode(luma, "420", quality=85, chroma=(blocks(), blocks()))
    Cc, st = JC.decode_color(data, (sw, sh))
    assert st == J.OK
    det = detector(W, H, 2)
    det.upload_jpeg([data, data], o, color=True)
    rgb = det.blob_rgb([0, 1])
    assert np.array_equal(rgb[0], NB.ycc_rgb(JC.preview_triples(Cc, o, W, H))) and np.array_equal(rgb[0], rgb[1])
    pp = B.blob_params([B.ColorClass(h_min=100, h_max=20, min_area=4), B.ColorClass(h_min=21, h_max=99, min_area=4)], erode=1, dilate=1)
    got = det.detect_blobs(pp, [1, 0])
    same(got, B.blobs_host(pp, rgb))
    assert got[1].sum() > 0
    det.close()


# ---- device mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(16, 16), (33, 17), (64, 48), (130, 33), (257, 65)])
def test_mask_equals_the_twin(B, W, H):
    """Both stages, four classes, every morphology depth pair of (0, 1, 4) x (0, 2); 257 x 65 is more than one wave of the
    threshold and more than one workgroup of the word kernels in both directions, its last word holds one pixel."""
    rng = np.random.default_rng(W * 7 + H)
    base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    blobby = np.kron(rng.integers(0, 2, ((H + 5) // 6, (W + 5) // 6)), np.ones((6, 6), int))[:H, :W].astype(bool)
    pics = [base, np.where(blobby[..., None], base | 0xC0, base >> 2).astype(np.uint8)]
    det = detector(W, H, 2)
    det.upload_raw([raw_of(p, "BGR3", "rotate-180") for p in pics], "BGR3", "rotate-180")
    rgb = det.blob_rgb([0, 1])
    assert np.array_equal(rgb, np.stack(pics))
    classes = [B.ColorClass(h_min=20, h_max=100), B.ColorClass(h_min=160, h_max=15), B.ColorClass(s_min=0, v_min=0),
               B.ColorClass(h_min=90, h_max=90, s_min=255, v_min=255)]
    for e in (0, 1, 4):
        for d in (0, 2):
            pp = B.blob_params(classes, erode=e, dilate=d)
            for c in range(4):
                for stage in (0, 1):
                    assert np.array_equal(det.blob_mask(pp, c, stage, [1, 0]), B.mask_host(pp, rgb[::-1], c, stage)), (e, d, c, stage)
    det.close()


# ---- device records ----------------------------------------------------------------------------------------------------------------
def seam_patterns(H, W):
    """The host patterns at a size where each crosses every word seam (x = 32, 64, ...) and many rows, corners included."""
    import test_blobs_host as TH
    yy, xx = np.mgrid[:H, :W]
    out = dict(TH.patterns(H, W))
    # a staircase of 2 x 1 steps that climbs through the corners (31, y) -> (32, y + 1) of the seams, and its mirror
    out["steps"] = (xx // 2 == yy) | ((W - 1 - xx) // 2 == yy)
    # diagonal pixels only, touching at corners, exactly across x = 31 | 32 and x = 63 | 64
    out["corners"] = ((xx - yy) % 32 == 0) & (yy < 40)
    # runs that end at bit 31 above runs that start at bit 0 and the other way round
    z = np.zeros((H, W), bool); z[0::4, 20:32] = True; z[1::4, 32:40] = True; z[2::4, 60:64] = True; z[3::4, 64:65] = True
    out["seam_touch"] = z
    return out


def test_records_equal_the_twin_on_the_patterns(B):
    H, W = 45, 100
    pats = seam_patterns(H, W)
    names = list(pats)
    det = detector(W, H, 4)
    cls = B.ColorClass(min_area=1, **ORANGE)
    pp = B.blob_params([cls], max_targets=64)
    for k in range(0, len(names), 4):
        group = names[k:k + 4]
        pics = [paint(pats[nm]) for nm in group]
        det.upload_raw([raw_of(p) for p in pics], "RGB3")
        idx = list(range(len(group)))
        rgb = det.blob_rgb(idx)
        assert np.array_equal(rgb, np.stack(pics))
        got = det.detect_blobs(pp, idx)
        same(got, B.blobs_host(pp, rgb), group)
        for i, nm in enumerate(group):   # and against scipy directly
            want, wc, ws = NB.detect([cls], pics[i], max_targets=64)
            assert list(got[1][i]) == wc and int(got[2][i]) == ws, nm
            assert [int(a) for a in got[0][i, 0, :len(want[0])]["area"]] == [r["area"] for r in want[0]], nm
    det.close()


def test_four_classes_repeated_index_three_sources(B):
    """Four classes at once, frames with a repeated index, morphology on, a camera and a mount; the same bytes from the handle's raw
    staging, the caller's device memory and a raw ring; two consecutive calls return identical bytes."""
    import torch
    from chalkydri_amd.camera import make_camera
    from chalkydri_amd.detector import IngestRing
    W, H, o, fourcc = 130, 75, "counterclockwise", "YUYV"
    sw, sh = R.source_size(W, H, o)
    rng = np.random.default_rng(12)
    ms = R.min_stride(fourcc, sw)
    raw = []
    for _ in range(3):   # patches of one (Y, U, Y, V) per 8 rows x 8 pixels: saturated colours of some size
        base = rng.integers(0, 256, ((sh + 7) // 8, (ms + 15) // 16, 1, 4), dtype=np.uint8)
        f = np.repeat(np.tile(base, (1, 1, 4, 1)).reshape(base.shape[0], -1), 8, axis=0)
        raw.append(np.ascontiguousarray(f[:sh, :ms]))
    cam = make_camera("EUCM", 110.0, 111.0, 64.5, 37.0, 0.6, 1.1)
    a = np.radians(20.0)
    Rm = np.array([[0.0, -1.0, 0.0], [-np.sin(a), 0.0, -np.cos(a)], [np.cos(a), 0.0, -np.sin(a)]])
    w = np.sqrt(1 + np.trace(Rm)) / 2
    mount = (list(-Rm @ np.array([0.0, 0.0, 0.5])), [w, (Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w)])
    classes = [B.ColorClass(h_min=170, h_max=15, min_area=6), B.ColorClass(h_min=30, h_max=80, min_area=6, ground_z=0.05),
               B.ColorClass(h_min=90, h_max=130, min_area=6, min_fill_permille=400), B.ColorClass(h_min=131, h_max=169, min_area=6, max_aspect_permille=3000)]
    pp = B.blob_params(classes, erode=1, dilate=2, camera=cam, robot_to_cam=mount)
    idx = [2, 0, 2, 1]
    det = detector(W, H, 4)
    det.upload_raw(raw, fourcc, o)
    rgb = det.blob_rgb(idx)
    want = B.blobs_host(pp, rgb)
    assert want[1].sum() >= 4 and (want[0]["flags"] & A.CK_BLOB_HAS_BEARING).any()
    got = det.detect_blobs(pp, idx)
    same(got, want, ["staged"])
    same(det.detect_blobs(pp, idx), got, ["second call"])
    dev = device_frames(torch, raw, ms, ms * sh, sh)
    same(det.detect_blobs_device(pp, dev.data_ptr() + 3, 3, ms, ms * sh, fourcc, o, frames=idx), want, ["device"])
    ring = IngestRing(det, 2, fourcc=fourcc, orientation=o)
    for i, f in enumerate(raw):
        ring.write(1, i, f)
    ring.submit(1, 3)
    same(ring.detect_blobs(1, pp, idx), want, ["ring"])
    # the handle's camera comes before the params': the twin given that camera agrees
    cam2 = make_camera("EUCM", 100.0, 100.0, 60.0, 40.0, 0.5, 1.0)
    det.set_camera(cam2)
    same(det.detect_blobs(pp, idx), B.blobs_host(B.blob_params(classes, erode=1, dilate=2, camera=cam2, robot_to_cam=mount), rgb), ["handle camera"])
    ring.close()
    det.close()


def test_overflow_truncation_and_cap(B):
    H, W = 45, 100
    yy, xx = np.mgrid[:H, :W]
    iso = (xx % 2 == 0) & (yy % 2 == 0)          # the worst case for a labelling: every other pixel a component of its own
    n_iso = int(iso.sum())
    det = detector(W, H, 2)
    det.upload_raw([raw_of(paint(iso)), raw_of(paint(~iso & (yy % 2 == 0)))], "RGB3")
    rgb = det.blob_rgb([0, 1])
    cls = B.ColorClass(min_area=1, **ORANGE)
    for maxc, cap, mt in ((n_iso - 1, 8, 8), (n_iso, 8, 8), (4096, 3, 16), (4096, 16, 2), (4096, 0, 16), (1, 4, 4), (W * H, 4, 4)):
        pp = B.blob_params([cls], max_components=maxc, max_targets=mt)
        got = det.detect_blobs(pp, [0, 1], cap=cap)
        same(got, B.blobs_host(pp, rgb, cap), (maxc, cap, mt))
        if maxc < n_iso:
            assert got[2][0] == A.CK_BLOB_OVERFLOW and got[1][0, 0] == 0 and not got[0][0].tobytes().strip(b"\0")
        else:
            assert got[2][0] == A.CK_BLOB_TRUNCATED and got[1][0, 0] == n_iso
    det.close()


def test_blob_calls_leave_the_detector_alone(B):
    """detect_batch before and after a blob call returns the same detections, and the staged luma is unchanged."""
    from chalkydri_amd import scenes
    W, H = 320, 240
    frames = scenes.bench_stream(3, 2, W, H, 2)[0]
    det = detector(W, H, 2)
    pics = []
    for f in frames:   # the tag scene in grey with a planted orange rectangle
        p = np.stack([f, f, f], -1)
        p[20:50, 30:90] = (255, 90, 0)
        pics.append(p)
    det.upload_raw([raw_of(p) for p in pics], "RGB3")
    luma0 = det.preview_luma([0, 1], width=0, height=0)
    key = lambda dets: [[(d.id(), d.corners().tobytes()) for d in f] for f in dets]
    before = key(det.detect_batch(None, n=2))
    pp = B.blob_params([B.ColorClass(h_min=5, h_max=25, min_area=50)], erode=1, dilate=1)
    got = det.detect_blobs(pp, [0, 1])
    assert list(got[1][:, 0]) == [1, 1] and got[0][0, 0, 0]["area"] == 30 * 60
    assert np.array_equal(det.preview_luma([0, 1], width=0, height=0), luma0)
    assert key(det.detect_batch(None, n=2)) == before and sum(len(f) for f in before) > 0
    same(det.detect_blobs(pp, [0, 1]), got)      # and the colour source is still there after a detect
    det.close()


def test_apriltags_task_reports_blobs(B):
    """AprilTags(..., blobs=...): the tag pose it returned without, and the planted rectangle as one target with a ground point
    that the task's own mount and calib explain."""
    from chalkydri_amd import scenes
    from chalkydri_amd.apriltags import AprilTags
    W, H = 320, 240
    frames, gyro, layout, calib, r2c = scenes.bench_stream(1, 1, W, H, 4)
    p = np.stack([frames[0]] * 3, -1)
    x0, x1, y0, y1 = 200, 239, 180, 199                     # below the horizon of a level camera 0.6 m up
    p[y0:y1 + 1, x0:x1 + 1] = (255, 90, 0)
    raw = [raw_of(p)]
    plain = AprilTags(W, H, layout, calib, r2c, cam_id=1, fourcc="RGB3")
    rec0, valid0 = plain.process_raw_batch(raw, list(gyro))
    assert plain.blobs is None
    task = AprilTags(W, H, layout, calib, r2c, cam_id=1, fourcc="RGB3", blobs=[B.ColorClass(h_min=5, h_max=25, min_area=100)])
    rec, valid = task.process_raw_batch(raw, list(gyro))
    assert list(valid) == list(valid0) and bytes(rec[0]) == bytes(rec0[0]) and valid[0]
    records, counts, status = task.blobs
    assert counts.tolist() == [[1]] and status.tolist() == [0]
    r = records[0, 0, 0]
    assert (r["x0"], r["y0"], r["x1"], r["y1"], r["area"]) == (x0, y0, x1, y1, 40 * 20)
    assert r["flags"] == A.CK_BLOB_HAS_BEARING | A.CK_BLOB_HAS_GROUND
    m = calib["OpenCVModel5"]
    # a level pinhole 0.6 m up at x = 0.2: the floor point under pixel (u, v) is fy * 0.6 / (v - cy) ahead and (u - cx) / fx of that to the right
    fwd = m["fy"] * r2c["z"] / (y1 + 1 - m["cy"])
    want = (r2c["x"] + fwd, r2c["y"] - fwd * ((x0 + x1 + 1) / 2.0 - m["cx"]) / m["fx"])
    assert np.allclose(r["ground"], want, rtol=1e-9, atol=1e-9)
    same(task.blobs, B.blobs_host(task._blob_params, task.detector.blob_rgb([0])))
    plain.detector.close()
    task.detector.close()


def test_blob_time_runs(B):
    import torch
    W, H, n = 64, 48, 2
    det = detector(W, H, n)
    raw = [PC.pack_colour(np.random.default_rng(i), "YUYV", W, H) for i in range(n)]
    dev = device_frames(torch, raw, 2 * W, 2 * W * H, H)
    ms = det.blob_time(B.blob_params(), dev.data_ptr() + 3, n, 2 * W, 2 * W * H, "YUYV", reps=3)
    assert 0.0 < ms < 1000.0
    det.close()


def test_cpp_blobs_demo(B, tmp_path):
    """include/chalkydri.hpp: BlobParams, detect_blobs, Handle::detect_blobs through tests/cpp/blobs_demo.cpp."""
    W, H, n = 66, 49, 2
    rng = np.random.default_rng(4)
    pics = []
    for _ in range(n):
        m = np.zeros((H, W), bool)
        for _ in range(4):
            x, y = int(rng.integers(0, W - 12)), int(rng.integers(0, H - 9))
            m[y:y + int(rng.integers(3, 9)), x:x + int(rng.integers(3, 12))] = True
        pics.append(paint(m))
    (tmp_path / "in.bin").write_bytes(b"".join(raw_of(p, "BGRA", "clockwise").tobytes() for p in pics))
    r = subprocess.run([DEMO, "BGRA", "1", str(W), str(H), str(n), "0", "20", "100", "100", "4", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["OK", str(n * 16), "16"], (r.stdout, r.stderr)
    pp = B.blob_params([B.ColorClass(h_min=0, h_max=20, s_min=100, v_min=100, min_area=4)])
    want = B.blobs_host(pp, np.stack(pics[::-1]))
    assert (tmp_path / "out.bin").read_bytes() == want[0].tobytes() + want[1].tobytes() + want[2].tobytes()
    assert want[1].sum() >= 2


def test_stress_small(B):
    import stress_blobs
    targets, flagged = stress_blobs.run(40, 7)
    assert targets > 0
