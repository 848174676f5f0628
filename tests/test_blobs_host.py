"""The coloured-piece detector without a device: the tuning helper and the host twin against tests/np_blobs.py, the
numpy / scipy restatement written from the definition; the filter's and the capacity rule's edges; the ground point against the
geometry; the plumbing (parameter check, layouts, exports, kernel budgets, the sanitizer build of the twin)."""
import colorsys
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_blobs as NB  # noqa: E402
import np_calib  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "chalkydri_amd", "lib", "blobs_host_check")
INT_FIELDS = ("class_id", "area", "x0", "y0", "x1", "y1", "seed", "sx", "sy", "sxx", "sxy", "syy", "flags")
F64_FIELDS = ("cx", "cy", "major", "minor", "axis", "bearing", "ground")


@pytest.fixture(scope="module")
def B(built):
    from chalkydri_amd import blobs
    return blobs


def paint(mask, on=(255, 40, 0), off=(10, 10, 10)):
    """bool [H][W] -> rgb [H][W][3]: a saturated orange where the mask is set."""
    rgb = np.empty(mask.shape + (3,), np.uint8)
    rgb[...] = off
    rgb[mask] = on
    return rgb


ORANGE = dict(h_min=0, h_max=20, s_min=100, v_min=100)


def compare(B, classes, rgb, **kw):
    """The twin against the restatement on one frame: integers equal, doubles within 1e-12 relative.  Returns the twin's triple."""
    cam, mount = kw.pop("camera", None), kw.pop("mount", None)
    cap = kw.pop("cap", None)
    pp = B.blob_params(classes, camera=cam, robot_to_cam=mount, **kw)
    rec, counts, status = B.blobs_host(pp, rgb, cap)
    ncam = None if cam is None else (cam.model, list(cam.k))
    want, wcounts, wstatus = NB.detect(classes, rgb, cap=cap, camera=ncam, mount=mount, **kw)
    assert list(counts[0]) == wcounts and int(status[0]) == wstatus
    for c, rows in enumerate(want):
        got = rec[0, c]
        assert not got[len(rows):].tobytes().strip(b"\0"), "unwritten records are zero"
        for j, w in enumerate(rows):
            for f in INT_FIELDS:
                assert int(got[j][f]) == int(w[f]), (c, j, f, got[j][f], w[f])
            for f in F64_FIELDS:
                np.testing.assert_allclose(got[j][f], w[f], rtol=1e-12, atol=1e-12, err_msg=f"{c} {j} {f}")
    return rec, counts, status


# ---- HSV ---------------------------------------------------------------------------------------------------------------------------
def test_rgb_hsv_equals_the_restatement(B):
    """The full R x G plane for 16 values of B, and 10^6 random colours."""
    r, g = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for b in (0, 1, 2, 17, 63, 64, 100, 127, 128, 129, 180, 200, 253, 254, 255, 31):
        rgb = np.stack([r, g, np.full_like(r, b)], -1).astype(np.uint8)
        assert np.array_equal(B.rgb_hsv(rgb), NB.rgb_hsv(rgb)), b
    rgb = np.random.default_rng(1).integers(0, 256, (1000000, 3), dtype=np.uint8)
    assert np.array_equal(B.rgb_hsv(rgb), NB.rgb_hsv(rgb))


def test_rgb_hsv_against_colorsys(B):
    """Hue within 0.5 of colorsys' h x 180 (on the circle), S within 1 of its s x 255, V equal."""
    rgb = np.random.default_rng(2).integers(0, 256, (200000, 3), dtype=np.uint8)
    hsv = B.rgb_hsv(rgb).astype(np.float64)
    ref = np.array([colorsys.rgb_to_hsv(*(p / 255.0)) for p in rgb.astype(np.float64)])
    dh = np.abs(hsv[:, 0] - ref[:, 0] * 180.0)
    dh = np.minimum(dh, 180.0 - dh)
    chroma = rgb.max(1) != rgb.min(1)
    assert dh[chroma].max() <= 0.5 + 1e-9
    assert np.abs(hsv[:, 1] - ref[:, 1] * 255.0).max() <= 1.0
    assert np.array_equal(hsv[:, 2], rgb.max(1))


# ---- mask --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [16, 31, 32, 33, 64, 65, 130])
def test_mask_twin_equals_the_restatement(B, W):
    H, rng = 23, np.random.default_rng(W)
    # blobs of strong colours on a dim ground, so that erosion leaves something, and pure noise in a second frame
    base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    blobby = np.kron(rng.integers(0, 2, ((H + 5) // 6, (W + 5) // 6)), np.ones((6, 6), int))[:H, :W].astype(bool)
    frames = np.stack([base, np.where(blobby[..., None], base | 0xC0, base >> 2).astype(np.uint8)])
    ranges = [dict(h_min=20, h_max=100), dict(h_min=160, h_max=15), dict(h_min=0, h_max=179, s_min=0, v_min=0),
              dict(h_min=90, h_max=90, s_min=255, s_max=255, v_min=255)]   # unwrapped, wrapped, full, (nearly) empty
    classes = [B.ColorClass(**r) for r in ranges]
    for e in (0, 1, 2, 4):
        for d in (0, 1, 2, 4):
            pp = B.blob_params(classes, erode=e, dilate=d)
            for c, cls in enumerate(classes):
                m0 = np.stack([NB.class_mask(cls, f) for f in frames])
                assert np.array_equal(B.mask_host(pp, frames, c, 0), NB.pack(m0)), (e, d, c, 0)
                m1 = np.stack([NB.morph(m, e, d) for m in m0])
                assert np.array_equal(B.mask_host(pp, frames, c, 1), NB.pack(m1)), (e, d, c, 1)
    assert np.array_equal(B.unpack_mask(NB.pack(m0), W), m0)


# ---- records -----------------------------------------------------------------------------------------------------------------------
def spiral(H, W):
    """A one-pixel-wide path that winds inwards, one blank pixel between its arms."""
    m = np.zeros((H, W), bool)
    x, y, dx, dy = 1, 1, 1, 0
    m[y, x] = True
    while True:
        steps = 0
        while True:
            nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if not (1 <= nx < W - 1 and 1 <= ny < H - 1) or m[ny, nx] or (0 <= fx < W and 0 <= fy < H and m[fy, fx]):
                break
            x, y, steps = nx, ny, steps + 1
            m[y, x] = True
        if steps == 0:
            return m
        dx, dy = -dy, dx


def patterns(H=37, W=70):
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[:H, :W]
    out = {}
    blobs = np.zeros((H, W), bool)
    for _ in range(9):
        cx, cy, a, b = rng.integers(0, W), rng.integers(0, H), rng.integers(2, 9), rng.integers(2, 6)
        blobs |= ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1
    out["blobs"] = blobs
    out["spiral"] = spiral(H, W)
    comb = np.zeros((H, W), bool); comb[3, 2:W - 2] = True; comb[3:H - 3, 2:W - 2:2] = True
    out["comb"] = comb
    out["staircase"] = (xx == yy + 3) | ((W - 1 - xx) == yy)     # diagonal steps: only 8-connectivity joins them
    out["checkerboard"] = (xx + yy) % 2 == 0
    out["isolated"] = (xx % 2 == 0) & (yy % 2 == 0)
    out["full"] = np.ones((H, W), bool)
    out["empty"] = np.zeros((H, W), bool)
    return out


@pytest.mark.parametrize("name", list(patterns()))
def test_records_twin_equals_scipy(B, name):
    m = patterns()[name]
    cls = B.ColorClass(min_area=1, **ORANGE)
    rec, counts, status = compare(B, [cls], paint(m), max_targets=64, max_components=4096)
    if name in ("checkerboard", "full", "spiral", "comb"):
        assert counts[0, 0] == 1 and rec[0, 0, 0]["area"] == m.sum()
    if name == "staircase":
        assert counts[0, 0] == 1   # the two diagonals cross
    if name == "empty":
        assert counts[0, 0] == 0 and status[0] == 0
    if name == "isolated":
        assert counts[0, 0] == m.sum() and status[0] == NB.TRUNCATED


def test_four_classes_and_morphology(B):
    rng = np.random.default_rng(8)
    H, W = 40, 75
    hue = np.kron(rng.integers(0, 6, ((H + 7) // 8, (W + 7) // 8)), np.ones((8, 8), int))[:H, :W]
    pal = np.array([(250, 30, 20), (30, 240, 40), (20, 40, 250), (240, 230, 20), (12, 12, 12), (200, 200, 200)], np.uint8)
    rgb = pal[hue]
    rgb[rng.random((H, W)) < 0.03] = (0, 0, 0)   # pepper, which the morphology has to deal with
    classes = [B.ColorClass(h_min=170, h_max=10, min_area=4), B.ColorClass(h_min=50, h_max=70, min_area=4),
               B.ColorClass(h_min=110, h_max=130, min_area=4), B.ColorClass(h_min=20, h_max=40, min_area=4, ground_z=0.1)]
    for e, d in ((0, 0), (1, 1), (2, 1), (0, 2)):
        _, counts, _ = compare(B, classes, rgb, erode=e, dilate=d, max_targets=32)
    assert counts.sum() > 4


def test_overflow_rule(B):
    """More components of min_area and more than max_components: the flag, count 0, nothing written; one fewer: exact."""
    m = patterns()["isolated"]
    n = int(m.sum())
    cls = B.ColorClass(min_area=1, **ORANGE)
    rec, counts, status = compare(B, [cls], paint(m), max_targets=8, max_components=n - 1)
    assert status[0] == NB.OVERFLOW and counts[0, 0] == 0 and not rec.tobytes().strip(b"\0")
    rec, counts, status = compare(B, [cls], paint(m), max_targets=8, max_components=n)
    assert status[0] == NB.TRUNCATED and counts[0, 0] == n
    # components below min_area take no slot: with min_area 2 the isolated pixels never overflow
    big = m.copy(); big[10:14, 10:20] = True
    rec, counts, status = compare(B, [B.ColorClass(min_area=2, **ORANGE)], paint(big), max_components=1)
    assert status[0] == 0 and counts[0, 0] == 1


def test_truncation_and_cap(B):
    m = np.zeros((30, 60), bool)
    for i in range(5):
        m[2:4 + i, 2 + 10 * i:8 + 10 * i] = True   # five boxes, the later the larger
    cls = B.ColorClass(min_area=1, **ORANGE)
    rec, counts, status = compare(B, [cls], paint(m), max_targets=3)            # max_targets cuts
    assert counts[0, 0] == 5 and status[0] == NB.TRUNCATED and list(rec[0, 0]["area"]) == [36, 30, 24]
    rec, counts, status = compare(B, [cls], paint(m), max_targets=16, cap=2)    # the caller's cap cuts
    assert counts[0, 0] == 5 and status[0] == NB.TRUNCATED and list(rec[0, 0]["area"]) == [36, 30]
    rec, counts, status = compare(B, [cls], paint(m), max_targets=5, cap=5)     # neither
    assert counts[0, 0] == 5 and status[0] == 0
    # equal areas: the smaller seed first
    m = np.zeros((12, 40), bool); m[6:8, 30:33] = True; m[2:4, 20:23] = True; m[2:4, 3:6] = True
    rec, _, _ = compare(B, [cls], paint(m))
    assert list(rec[0, 0]["seed"][:3]) == [2 * 40 + 3, 2 * 40 + 20, 6 * 40 + 30]


def test_filter_edges(B):
    """Each of the four inequalities at equality and one off.  The piece: 10 x 4 box with 30 pixels (an L)."""
    m = np.zeros((20, 40), bool); m[5:9, 5:15] = True; m[5:7, 10:15] = False     # N = 30, bw = 10, bh = 4
    rgb = paint(m)

    def count(**kw):
        return int(compare(B, [B.ColorClass(**{**ORANGE, "min_area": 1, **kw})], rgb)[1][0, 0])
    assert count(min_area=30) == 1 and count(min_area=31) == 0
    assert count(max_area=30) == 1 and count(max_area=29) == 0 and count(max_area=0) == 1
    assert count(min_fill_permille=750) == 1 and count(min_fill_permille=751) == 0          # 1000 * 30 = 750 * 40
    assert count(min_aspect_permille=2500) == 1 and count(min_aspect_permille=2501) == 0    # 1000 * 10 = 2500 * 4
    assert count(max_aspect_permille=2500) == 1 and count(max_aspect_permille=2499) == 0 and count(max_aspect_permille=0) == 1


def test_axis_conventions(B):
    cls = B.ColorClass(min_area=1, **ORANGE)
    m = np.zeros((20, 20), bool); m[5:9, 5:9] = True             # isotropic: (1, 0)
    r = compare(B, [cls], paint(m))[0][0, 0, 0]
    assert tuple(r["axis"]) == (1.0, 0.0) and r["major"] == r["minor"]
    m[:] = False; m[3:17, 10] = True                             # vertical: (0, 1), first non-zero component positive
    r = compare(B, [cls], paint(m))[0][0, 0, 0]
    assert tuple(r["axis"]) == (0.0, 1.0) and r["minor"] == 0.0
    m[:] = False; m[np.arange(3, 15), 17 - np.arange(3, 15)] = True   # anti-diagonal: x positive, y negative
    r = compare(B, [cls], paint(m))[0][0, 0, 0]
    assert r["axis"][0] > 0 and r["axis"][1] < 0 and r["flags"] == 0
    m[:] = False; m[0:3, 4:9] = True
    assert compare(B, [cls], paint(m))[0][0, 0, 0]["flags"] == NB.AT_BORDER


# ---- ground point ------------------------------------------------------------------------------------------------------------------
def cameras():
    from chalkydri_amd.camera import make_camera
    k, w, h = np_calib.cameras()["cam2_1280x720"]     # the reference's calib blob (chalkydri.ron)
    yield "opencv5", make_camera("OpenCVModel5", *k), w, h
    yield "eucm", make_camera("EUCM", 420.0, 421.0, 641.5, 358.0, 0.62, 1.07), 1280, 720


# a camera 0.5 m up, looking along the robot's x, 20 degrees down.  Camera axes in the robot frame: z (forward) = (cos, 0, -sin),
# x (right) = (0, -1, 0), y (down) = (-sin, 0, -cos); the rows of R (cam from robot) are those axes, t = -R c.
def mount_down(degrees=20.0):
    a = np.radians(degrees)
    R = np.array([[0.0, -1.0, 0.0], [-np.sin(a), 0.0, -np.cos(a)], [np.cos(a), 0.0, -np.sin(a)]])
    c = np.array([0.0, 0.0, 0.5])
    w = np.sqrt(1 + np.trace(R)) / 2
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    assert np.allclose(NB.quat_mat(q), R)
    return R, (list(-R @ c), list(q))


@pytest.mark.parametrize("name,cam,W,H", list(cameras()), ids=lambda v: v if isinstance(v, str) else None)
def test_ground_point(B, name, cam, W, H):
    R, mount = mount_down()
    L = B._bind(B.lib())
    cls = B.ColorClass(min_area=1, **ORANGE)
    ncam = (cam.model, list(cam.k))
    for dist, side in ((1.0, 0.2), (3.0, -0.5), (6.0, 1.0)):
        floor = np.array([dist, side, 0.0])
        pc = R @ floor + np.array(mount[0])
        px, ok = np.zeros(2), C.c_uint8()
        assert L.ck_camera_project_host(C.byref(cam), pc.ctypes.data, 1, px.ctypes.data, C.byref(ok)) == 0 and ok.value
        # a box whose bottom centre ((x0 + x1 + 1) / 2, y1 + 1) is the pixel that holds the projection
        u, v = int(np.floor(px[0])), int(np.floor(px[1]))
        x0, x1, y1 = u - 3, u + 2, v - 1
        assert x0 >= 0 and x1 < W and 8 <= y1 < H
        m = np.zeros((H, W), bool); m[y1 - 7:y1 + 1, x0:x1 + 1] = True
        rec, counts, _ = compare(B, [cls], paint(m), camera=cam, mount=mount)
        r = rec[0, 0, 0]
        assert counts[0, 0] == 1 and r["flags"] & NB.HAS_GROUND and r["flags"] & NB.HAS_BEARING
        want = NB.ground_point(ncam, mount, 0.0, 20.0, (x0 + x1 + 1) / 2.0, y1 + 1.0)
        assert np.abs(r["ground"] - want).max() <= 1e-9
        # the true point lies in the pixel below the box, so the report is off by less than what the rays of that pixel's two
        # vertical neighbours (the rows above and below it) span on the ground
        g_up = NB.ground_point(ncam, mount, 0.0, 1e9, px[0], v - 1.0)
        g_dn = NB.ground_point(ncam, mount, 0.0, 1e9, px[0], v + 2.0)
        tol = np.linalg.norm(g_up - g_dn)
        assert np.linalg.norm(r["ground"] - floor[:2]) <= tol, (name, dist, r["ground"], tol)
    # a box that ends at or above the horizon has no ground point; neither has one beyond max_range
    # (from a mount 5 degrees down, so that the horizon is inside both cameras' frames)
    R5, mount5 = mount_down(5.0)
    for above, has in ((2.0, False), (0.0, False), (-2.0, True)):       # degrees above the horizon; at it the ray is level: none
        hz = R5 @ np.array([50.0, 0.0, 0.5 + 50.0 * np.tan(np.radians(above))]) + np.array(mount5[0])
        px, ok = np.zeros(2), C.c_uint8()
        assert L.ck_camera_project_host(C.byref(cam), hz.ctypes.data, 1, px.ctypes.data, C.byref(ok)) == 0 and ok.value
        u, v = int(round(px[0])), int(round(px[1]))
        assert 8 <= v < H
        m = np.zeros((H, W), bool); m[v - 8:v, u - 3:u + 3] = True       # bottom centre (u, v): the ray to that very point
        r = compare(B, [cls], paint(m), camera=cam, mount=mount5, max_range=1e6)[0][0, 0, 0]
        assert r["area"] == 48 and r["flags"] & NB.HAS_BEARING
        if above != 0.0:   # (at the horizon itself the rounding to a pixel decides: the restatement is the check there)
            assert bool(r["flags"] & NB.HAS_GROUND) == has and (has or tuple(r["ground"]) == (0.0, 0.0))
    far = R @ np.array([6.0, 0.0, 0.0]) + np.array(mount[0])
    assert L.ck_camera_project_host(C.byref(cam), far.ctypes.data, 1, px.ctypes.data, C.byref(ok)) == 0 and ok.value
    u, v = int(px[0]), int(px[1])
    m = np.zeros((H, W), bool); m[v - 8:v, u - 3:u + 3] = True
    assert compare(B, [cls], paint(m), camera=cam, mount=mount, max_range=7.0)[0][0, 0, 0]["flags"] & NB.HAS_GROUND
    assert not compare(B, [cls], paint(m), camera=cam, mount=mount, max_range=5.0)[0][0, 0, 0]["flags"] & NB.HAS_GROUND
    # without a mount: the bearing alone
    r = compare(B, [cls], paint(m), camera=cam)[0][0, 0, 0]
    assert r["flags"] == NB.HAS_BEARING and abs(np.linalg.norm(r["bearing"]) - 1) < 1e-12


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def test_check_error_order(B):
    """ck_blob_check refuses each bad field; with several bad fields the documented order decides which is met first — observable
    only as CK_EINVAL either way, so the order is checked by making each field in turn the ONLY bad one and by the null pointer."""
    L = B._bind(B.lib())
    assert L.ck_blob_check(None) == A.CK_EINVAL
    good = lambda: B.blob_params([B.ColorClass(), B.ColorClass()])
    assert L.ck_blob_check(C.byref(good())) == A.CK_OK
    for field, bad in (("n_classes", 0), ("n_classes", 5), ("erode", -1), ("erode", 5), ("dilate", -1), ("dilate", 5), ("max_targets", -1),
                       ("max_components", 0), ("max_range", -1.0), ("max_range", float("nan"))):
        pp = good(); setattr(pp, field, bad)
        assert L.ck_blob_check(C.byref(pp)) == A.CK_EINVAL, (field, bad)
    for field, bad in (("h_min", -1), ("h_min", 180), ("h_max", 180), ("s_min", 256), ("s_max", -1), ("v_min", 256), ("v_max", 256),
                       ("min_area", -1), ("max_area", -1), ("min_fill_permille", -1), ("min_aspect_permille", -1),
                       ("max_aspect_permille", -1), ("ground_z", float("inf"))):
        pp = good(); setattr(pp.cls[1], field, bad)
        assert L.ck_blob_check(C.byref(pp)) == A.CK_EINVAL, (field, bad)
        pp = good(); pp.n_classes = 1; setattr(pp.cls[1], field, bad)     # a class beyond n_classes is not looked at
        assert L.ck_blob_check(C.byref(pp)) == A.CK_OK, (field, bad)
    pp = good(); pp.has_camera = 1                                         # an all-zero camera: fx = 0
    assert L.ck_blob_check(C.byref(pp)) == A.CK_EINVAL
    pp.cam.k[0] = pp.cam.k[1] = 100.0
    assert L.ck_blob_check(C.byref(pp)) == A.CK_OK
    pp.has_mount = 1; pp.robot_to_cam.q[0] = 0.0
    assert L.ck_blob_check(C.byref(pp)) == A.CK_EINVAL
    pp.robot_to_cam.q[2] = 2.0                                             # any length > 0
    assert L.ck_blob_check(C.byref(pp)) == A.CK_OK
    pp.robot_to_cam.t[1] = float("nan")
    assert L.ck_blob_check(C.byref(pp)) == A.CK_EINVAL
    rgb, out = np.zeros((1, 4, 4, 3), np.uint8), np.zeros(16, B.BLOB_DTYPE)
    cnt = np.zeros(4, np.int32)
    pp = good()
    assert L.ck_blobs_host(C.byref(pp), rgb.ctypes.data, 4, 4, 1, out.ctypes.data, -1, cnt.ctypes.data, None) == A.CK_EINVAL
    assert L.ck_blobs_host(C.byref(pp), rgb.ctypes.data, 0, 4, 1, out.ctypes.data, 1, cnt.ctypes.data, None) == A.CK_EINVAL
    assert L.ck_blobs_host(C.byref(pp), rgb.ctypes.data, 4, 4, 1, out.ctypes.data, 1, cnt.ctypes.data, None) == A.CK_OK
    assert L.ck_blob_mask_host(C.byref(pp), rgb.ctypes.data, 4, 4, 1, 2, 0, cnt.ctypes.data) == A.CK_EINVAL
    assert L.ck_blob_mask_host(C.byref(pp), rgb.ctypes.data, 4, 4, 1, 0, 2, cnt.ctypes.data) == A.CK_EINVAL


def test_layouts_exports_and_abi(B):
    assert C.sizeof(A.BlobClass) == 56 and A.BlobClass.ground_z.offset == 48
    assert C.sizeof(A.BlobParams) == 400 and A.BlobParams.cls.offset == 32 and A.BlobParams.cam.offset == 256
    assert A.BlobParams.robot_to_cam.offset == 336 and A.BlobParams.max_range.offset == 392
    assert C.sizeof(A.Blob) == 160 and A.Blob.seed.offset == 28 and A.Blob.sx.offset == 32 and A.Blob.cx.offset == 72
    assert A.Blob.axis.offset == 104 and A.Blob.bearing.offset == 120 and A.Blob.ground.offset == 144
    assert B.BLOB_DTYPE.fields["ground"][1] == 144 and B.BLOB_DTYPE.fields["sx"][1] == 32
    L = B.lib()
    for name in ("ck_blob_params_default", "ck_blob_check", "ck_blob_rgb_hsv", "ck_blob_mask_host", "ck_blobs_host", "ck_detect_blobs",
                 "ck_detect_blobs_device", "ck_detect_blobs_ingested", "ck_blob_rgb", "ck_blob_rgb_device", "ck_blob_mask",
                 "ck_blob_mask_device", "ck_blob_time"):
        assert hasattr(L, name), name
    assert L.ck_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "chalkydri_hip.h")).read()
    assert "#define CK_ABI_VERSION 3 " in hdr and "#define CK_BLOB_MAX_CLASSES 4" in hdr
    pp = B.blob_params()
    assert (pp.n_classes, pp.erode, pp.dilate, pp.max_targets, pp.max_components, pp.max_range) == (1, 0, 0, 16, 4096, 20.0)
    assert (A.CK_BLOB_HAS_BEARING, A.CK_BLOB_HAS_GROUND, A.CK_BLOB_AT_BORDER, A.CK_BLOB_TRUNCATED, A.CK_BLOB_OVERFLOW) == (1, 2, 4, 1, 2)


def test_blob_kernels_have_no_private_segment(built):
    """Every kernel of k_blobs.o: private segment 0 and no vector-register spill, from the code object's own notes."""
    import shutil
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    res = {}
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(os.path.join(ROOT, "chalkydri_amd", "csrc", "build", "k_blobs.o"), td)
        subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", "k_blobs.o"], cwd=td, stdout=subprocess.DEVNULL)
        co = [f for f in os.listdir(td) if f.startswith("k_blobs.o") and "amdgcn" in f][0]
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], cwd=td, text=True)
    name = None
    for line in notes.splitlines():
        m = re.match(r"\s*\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.match(r"\s*\.(vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    for frag in ("k_blob_rgb", "k_blob_jrgb", "k_blob_mask", "k_blob_jmask", "k_blob_morph", "k_blob_init", "k_blob_merge",
                 "k_blob_flatten", "k_blob_slots", "k_blob_sums", "k_blob_final"):
        assert any(frag in k for k in res), frag
    for k, v in res.items():
        assert v == {"vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (k, v)


def test_blobs_demo_is_built(built):
    demo = os.path.join(ROOT, "chalkydri_amd", "lib", "blobs_demo")
    assert os.path.exists(demo)
    r = subprocess.run([demo], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


def test_host_twin_under_sanitizers(built):
    """csrc/ck_blobs_host.c alone under AddressSanitizer + UBSan, driven by tests/cpp/blobs_host_check.cpp."""
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "blobs_host_check ok" in r.stdout
