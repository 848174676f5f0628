"""Camera models on the host (ck_camera_host.c, chalkydri_amd/camera.py): EUCM / UCM projection and unprojection against
the independent numpy restatement (tests/np_camera.py), the exact identities the device path relies on (alpha = 0 is the pinhole, UCM
is EUCM with beta = 1, OpenCVModel5 is the fixed-point iteration of tests/np_tag_pose.py), the valid disc, the refusals, the blob
loader, the host half under sanitizers and the unprojection kernels' register / scratch figures.  No device needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_camera as NC  # noqa: E402
import np_tag_pose as NT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "chalkydri_amd", "lib", "camera_host_check")


@pytest.fixture(scope="module")
def cam(built):
    from chalkydri_amd import camera
    return camera


def _lens_camera(cam, name):
    lens = NC.LENSES[name]
    return cam.make_camera("UCM", *lens[:5]) if name == "ucm" else cam.make_camera("EUCM", *lens)


@pytest.mark.parametrize("name", sorted(NC.LENSES))
def test_host_agrees_with_the_restatement(cam, name):
    """A 16-px grid over 1280 x 800.  Bounds: some tens of ulps of unit-size (bearings, 1e-14) and 1e3-size (pixels, 1e-10) doubles
    over a dozen operations; project(unproject(px)) = px to 1e-9 px (numpy on the wide lens: 2.3e-13, every grid pixel valid)."""
    lens, c, px = NC.LENSES[name], _lens_camera(cam, name), NC.grid()
    b, ok = cam.unproject_host(c, px)
    bw, okw = NC.unproject(lens, px)
    assert okw.all() and np.array_equal(ok, okw)
    print(name, "bearing diff", np.abs(b - bw).max(), "widest", NC.off_axis_deg(lens, px).max(), "deg")
    assert np.abs(b - bw).max() <= 1e-14
    xy, okn = cam.normalize_host(c, px)
    xyw, oknw = NC.normalize(lens, px)
    assert np.array_equal(okn, oknw) and np.abs(xy - xyw)[okn].max() <= 1e-12 * max(1.0, np.abs(xyw).max())
    # projection of points at mixed depths along the restatement's bearings
    pts = bw * (0.3 + np.arange(len(bw)) % 7)[:, None]
    uv, okp = cam.project(c, pts)
    uvw, okpw = NC.project(lens, pts)
    assert okpw.all() and np.array_equal(okp, okpw)
    print(name, "pixel diff", np.abs(uv - uvw).max())
    assert np.abs(uv - uvw).max() <= 1e-10
    back, okb = cam.project(c, b)
    print(name, "round trip", np.abs(back - px).max())
    assert okb.all() and np.abs(back - px).max() <= 1e-9


def test_alpha_zero_is_the_pinhole_byte_for_byte(cam):
    """alpha = 0: kz == 1.0 exactly, the bearing is OpenCVModel5's with zero distortion (its first fixed-point step is exact), whatever
    beta is: the identity the device tests of ck_set_camera rely on."""
    px = NC.grid(16) + 0.37
    p5 = cam.make_camera("OpenCVModel5", 612.5, 609.25, 641.3, 398.7, 0, 0, 0, 0, 0)
    b5, ok5 = cam.unproject_host(p5, px)
    n5, okn5 = cam.normalize_host(p5, px)
    for beta in (1.0, 1.08, 0.7):
        e = cam.make_camera("EUCM", 612.5, 609.25, 641.3, 398.7, 0.0, beta)
        b, ok = cam.unproject_host(e, px)
        assert b.tobytes() == b5.tobytes() and np.array_equal(ok, ok5) and ok.all()
        n, okn = cam.normalize_host(e, px)
        assert n.tobytes() == n5.tobytes() and np.array_equal(okn, okn5)
    u = cam.make_camera("UCM", 612.5, 609.25, 641.3, 398.7, 0.0)
    assert cam.unproject_host(u, px)[0].tobytes() == b5.tobytes()


def test_ucm_is_eucm_with_beta_one_byte_for_byte(cam):
    from chalkydri_amd import _abi as A
    px = NC.grid(16) - 0.21
    e = cam.make_camera("EUCM", 700, 700, 630, 410, 0.55, 1.0)
    u = A.Camera()
    u.model = A.CK_CAMERA_UCM
    for i, v in enumerate((700, 700, 630, 410, 0.55, -7.5)):      # k[5] is read as 1.0 whatever it holds
        u.k[i] = v
    for fn in (cam.unproject_host, cam.normalize_host):
        a, oka = fn(e, px)
        b, okb = fn(u, px)
        assert a.tobytes() == b.tobytes() and np.array_equal(oka, okb)
    pts = cam.unproject_host(e, px)[0] * 2.5
    assert cam.project(e, pts)[0].tobytes() == cam.project(u, pts)[0].tobytes()


def test_opencv5_host_path_is_the_fixed_point_iteration(cam):
    """The host's OpenCVModel5 against tests/np_tag_pose.py's restatement of the 50-step iteration, pixels that do not converge among
    them (a strong barrel distortion far outside the image)."""
    k = (900.0, 905.0, 640.0, 400.0, -0.28, 0.07, 1e-3, -2e-4, 0.01)
    c = cam.make_camera("OpenCVModel5", *k)
    px = np.concatenate([NC.grid(32), [[9000.0, 7000.0], [-5000.0, 400.0], [640.0, 400.0]]])
    x, y, conv = NT.undistort(k, px[:, 0], px[:, 1])
    xy, ok = cam.normalize_host(c, px)
    assert np.array_equal(ok, conv) and conv.sum() >= len(px) - 2 and not conv.all()
    assert np.array_equal(xy[ok, 0], x[ok]) and np.array_equal(xy[ok, 1], y[ok])
    b, okb = cam.unproject_host(c, px)
    nrm = np.sqrt(x * x + y * y + 1.0)
    assert np.array_equal(okb, conv) and np.array_equal(b[ok], np.stack([x / nrm, y / nrm, 1.0 / nrm], 1)[ok])


def test_valid_disc_and_cone(cam):
    lens = NC.LENSES["eucm_wide"]
    fx, fy, cx, cy, alpha, beta = lens
    c = _lens_camera(cam, "eucm_wide")
    r = np.sqrt(1.0 / (beta * (2 * alpha - 1)))
    ang = np.linspace(0, 2 * np.pi, 37)[:-1]
    ring = lambda s: np.stack([cx + fx * s * r * np.cos(ang), cy + fy * s * r * np.sin(ang)], 1)
    for s, want in ((1.0 + 1e-9, False), (1.5, False), (1.0 - 1e-9, True), (0.5, True)):
        b, ok = cam.unproject_host(c, ring(s))
        assert (ok == want).all(), s
        assert np.array_equal(ok, NC.unproject(lens, ring(s))[1])
        if not want:
            assert not b.any()
    # just inside the disc the ray points backwards: a bearing, but no normalised point (the per-tag pose refuses the tag)
    b, ok = cam.unproject_host(c, ring(0.999))
    xy, okn = cam.normalize_host(c, ring(0.999))
    assert ok.all() and (b[:, 2] < 0).all() and not okn.any() and not xy.any()
    # kz = 0 lies at r2 = 1 / (alpha^2 beta): forward inside, backward outside
    r0 = np.sqrt(1.0 / (alpha * alpha * beta)) / r
    assert cam.normalize_host(c, ring(r0 * 0.999))[1].all() and not cam.normalize_host(c, ring(r0 * 1.001))[1].any()
    # projection: Z > -w d with w = (1 - alpha) / alpha
    w = (1 - alpha) / alpha
    rho = np.array([1.0, 0.3, 2.0])
    for f, want in ((0.99, True), (1.01, False)):
        z = -f * w * np.sqrt(beta * rho * rho / (1 - (f * w) ** 2))      # Z = -f w d on a cone of its own
        pts = np.stack([rho, 0 * rho, z], 1)
        uv, ok = cam.project(c, pts)
        assert (ok == want).all() and np.array_equal(ok, NC.project(lens, pts)[1]), f
    # alpha <= 0.5: every pixel is valid
    assert cam.unproject_host(_lens_camera(cam, "eucm_mild"), ring(40.0))[1].all()


def test_camera_check_refusals_in_order(cam):
    from chalkydri_amd import _abi as A
    from chalkydri_amd._lib import lib
    from chalkydri_amd.detector import _bind
    L = _bind(lib())

    def rc(model, k):
        c = A.Camera()
        c.model = model
        for i, v in enumerate(k):
            c.k[i] = v
        return L.ck_camera_check(C.byref(c))
    good = [500, 502, 640, 400, 0.62, 1.08, 0, 0, 0]
    nan, inf = float("nan"), float("inf")
    assert L.ck_camera_check(None) == A.CK_EINVAL                                   # a null pointer
    assert rc(3, good) == A.CK_EINVAL and rc(-1, good) == A.CK_EINVAL               # an unknown model
    assert rc(A.CK_CAMERA_EUCM, good) == A.CK_OK and rc(A.CK_CAMERA_UCM, good) == A.CK_OK
    for i in range(9):                                                              # a parameter that is not finite
        for bad in (nan, inf, -inf):
            k = list(good)
            k[i] = bad
            for model in (A.CK_CAMERA_OPENCV5, A.CK_CAMERA_EUCM):
                assert rc(model, k) == A.CK_EINVAL, (i, bad, model)
            assert rc(A.CK_CAMERA_UCM, k) == (A.CK_OK if i == 5 else A.CK_EINVAL)   # (UCM's k[5] is never looked at)
    for i in (0, 1):                                                                # fx, fy <= 0
        for bad in (0.0, -500.0):
            k = list(good)
            k[i] = bad
            assert all(rc(m, k) == A.CK_EINVAL for m in (0, 1, 2))
    for a in (-1e-9, 1.0 + 1e-9):                                                   # alpha outside [0, 1]
        assert rc(1, good[:4] + [a] + good[5:]) == A.CK_EINVAL and rc(2, good[:4] + [a] + good[5:]) == A.CK_EINVAL
    assert rc(1, good[:4] + [0.0] + good[5:]) == A.CK_OK and rc(1, good[:4] + [1.0] + good[5:]) == A.CK_OK
    for b in (0.0, -1.0):                                                           # beta <= 0
        assert rc(1, good[:5] + [b, 0, 0, 0]) == A.CK_EINVAL and rc(2, good[:5] + [b, 0, 0, 0]) == A.CK_OK
    for i in (6, 7, 8):                                                             # a non-zero unused slot
        k = list(good)
        k[i] = 1e-12
        assert rc(1, k) == A.CK_EINVAL and rc(2, k) == A.CK_EINVAL and rc(0, k) == A.CK_OK
    # OpenCVModel5 takes what it always took: any finite distortion
    assert rc(0, [900, 900, 640, 400, -0.3, 5.0, 0.1, -0.1, 2.0]) == A.CK_OK
    # the array entry points: the camera first, then the arrays
    px, out, ok = np.zeros((4, 2)), np.zeros((4, 3)), np.zeros(4, np.uint8)
    c = cam.make_camera("EUCM", *good[:6])
    for fn in (L.ck_camera_unproject_host, L.ck_camera_normalize_host, L.ck_camera_project_host, L.ck_camera_unproject):
        assert fn(None, out.ctypes.data, 4, out.ctypes.data, ok.ctypes.data) == A.CK_EINVAL
        assert fn(C.byref(c), None, 4, out.ctypes.data, ok.ctypes.data) == A.CK_EINVAL
        assert fn(C.byref(c), out.ctypes.data, 4, None, ok.ctypes.data) == A.CK_EINVAL
        assert fn(C.byref(c), out.ctypes.data, 4, out.ctypes.data, None) == A.CK_EINVAL
        assert fn(C.byref(c), out.ctypes.data, -1, out.ctypes.data, ok.ctypes.data) == A.CK_EINVAL
    assert L.ck_set_camera(None, C.byref(c)) == A.CK_EINVAL and L.ck_set_camera(None, None) == A.CK_EINVAL      # a null handle
    del px


def test_loader_reads_the_three_schemas(cam):
    from chalkydri_amd import _abi as A
    o5 = dict(fx=1368.3, fy=1368.5, cx=784.1, cy=655.2, k1=-0.03, k2=-0.002, p1=-0.001, p2=-0.0001, k3=0.015, width=1600, height=1304)
    c = cam.camera_from_calib({"OpenCVModel5": o5})
    assert c.model == A.CK_CAMERA_OPENCV5 and list(c.k) == [o5[f] for f in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]
    e = dict(fx=500, fy=502, cx=640, cy=400, alpha=0.62, beta=1.08, width=1280, height=800)
    c = cam.camera_from_calib({"EUCM": e})
    assert c.model == A.CK_CAMERA_EUCM and list(c.k) == [500, 502, 640, 400, 0.62, 1.08, 0, 0, 0]
    import json
    c = cam.camera_from_calib(json.dumps({"UCM": dict(fx=700, fy=700, cx=630, cy=410, alpha=0.55, width=1280, height=800)}))
    assert c.model == A.CK_CAMERA_UCM and list(c.k) == [700, 700, 630, 410, 0.55, 1.0, 0, 0, 0]
    assert cam.calib_from_camera(cam.camera_from_calib({"EUCM": e}), 1280, 800) == {"EUCM": {k: (float(v) if k not in ("width", "height") else v) for k, v in e.items()}}
    for blob in ({"KB4": e}, {"EUCMT": e}, {}, {"EUCM": e, "UCM": e}, [1, 2]):
        with pytest.raises(ValueError):
            cam.camera_from_calib(blob)
    with pytest.raises(ValueError):
        cam.camera_from_calib({"EUCM": dict(e, alpha=1.5)})
    with pytest.raises(KeyError):
        cam.camera_from_calib({"EUCM": {k: v for k, v in e.items() if k != "beta"}})


def test_host_half_under_sanitizers(built):
    """The three models over a pixel grid, the round trip, the identities, the disc and the refusals under AddressSanitizer + UBSan: a
    stand-alone program of ck_camera_host.c alone; it exits non-zero on the first finding of either sanitizer."""
    assert os.path.exists(CHECK)
    sym = subprocess.run(["nm", CHECK], capture_output=True, text=True).stdout
    assert "__asan_init" in sym and "__ubsan_handle" in sym          # the build that ran is the sanitized one
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def _notes(obj):
    llvm = "/opt/rocm/lib/llvm/bin"
    res = {}
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(obj, td)
        base = os.path.basename(obj)
        subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", base], cwd=td, stdout=subprocess.DEVNULL)
        co = [f for f in os.listdir(td) if f.startswith(base) and "amdgcn" in f][0]
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], cwd=td, text=True)
    name = None
    for line in notes.splitlines():
        m = re.match(r"\s*\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.match(r"\s*\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    return res


def test_unprojection_kernels_use_no_scratch(built):
    """The code object's own notes: the unprojection kernel and the glue (which now branches on the model) have no scratch and no
    spills; the per-tag pose kernel, whose every register counts (DESIGN.md §Per-tag pose), needs no more registers than before the
    branch: 304, read from a build of the commit before this one."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf in this image")
    build = os.path.join(ROOT, "chalkydri_amd", "csrc", "build")
    sq, tp = _notes(os.path.join(build, "k_sqpnp.o")), _notes(os.path.join(build, "k_tagpose.o"))
    for frag in ("k_camera_unproject", "k_glue", "k_unproject"):
        got = [v for k, v in sq.items() if frag in k]
        assert got, frag
        for v in got:
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (frag, v)
    got = [v for k, v in tp.items() if "k_tagpose" in k]
    assert got and all(v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 304 for v in got), got
