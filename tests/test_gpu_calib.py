"""The device solver of the camera calibration (k_calib.hip through ck_calib_refine_batch / ck_calibrate_batch) against
its bitwise specification ck_calib_refine_host: parameters, poses, costs, iterations and status compared as bytes.

Shapes, the smallest at which the kernel can still go wrong: F = 3 (fewer frames than the workgroup's 4 waves), F = 4 with 24, 63, 65
and 144 points per frame (below, at and above one round of 64 lanes, ragged; 24 = min_points_per_frame exactly), F = 9 (not a multiple
of the waves); free, frozen distortion, frozen focal lengths; max_iters = 3 (MAXIT)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_calib as N  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1600, 1304
SHAPES = {"F3": (144, 100, 80), "F4": (24, 63, 65, 144), "F9": (144, 30, 64, 128, 129, 77, 24, 143, 96)}
# (shape, fixed_mask, max_iters)
CASES = [("F3", 0, 100), ("F4", 0, 100), ("F4", A.CK_CALIB_FIX_DISTORTION, 100), ("F4", A.CK_CALIB_FIX_FOCAL, 100), ("F9", 0, 100), ("F4", 0, 3)]


def _frames(counts, seed):
    """Frames of the whole board (1.1-1.3 m away, centred: all 144 corners in view) at 0.1 px noise, cut to `counts` random corners."""
    k = N.cameras()["cam1_1600x1304"][0]
    rng = np.random.default_rng([seed, len(counts)])
    XY = N.board_points()
    out = []
    for n in counts:
        a, tilt, spin = rng.uniform(0, 2 * np.pi), rng.uniform(0.15, 0.5), rng.uniform(0, 2 * np.pi)
        R = N.rodrigues(tilt * np.array([np.cos(a), np.sin(a), 0.0])) @ N.rodrigues(np.array([0, 0, spin]))
        t = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(1.1, 1.3)]) - R[:, :2] @ XY.mean(0)
        uv = N.project(k, R, t, XY)
        assert uv.min() > 4 and (uv[:, 0] < W - 5).all() and (uv[:, 1] < H - 5).all()
        sel = np.sort(rng.choice(144, n, replace=False))
        out.append((XY[sel].copy(), uv[sel] + rng.normal(0, 0.1, (n, 2))))
    return out


@pytest.fixture(scope="module")
def K(built):
    from chalkydri_amd import calibration
    return calibration


@pytest.fixture(scope="module")
def det(built):
    from chalkydri_amd.detector import AprilTagDetector
    d = AprilTagDetector(640, 480)      # the calibration calls are not bound to the handle's geometry
    yield d
    d.close()


@pytest.fixture(scope="module")
def ref(K):
    """Per case: the frames, the start and the host twin's result, computed once and left unchanged."""
    out = {}
    for i, (shape, mask, iters) in enumerate(CASES):
        frames = _frames(SHAPES[shape], 40 + sorted(SHAPES).index(shape))
        p = K.params(W, H, fixed_mask=mask, max_iters=iters)
        cam0, poses0, st = K.calib_init(p, frames)
        assert st == A.CK_CALIB_CONVERGED
        res, poses = K.refine_host(p, frames, cam0, poses0)
        out[i] = dict(frames=frames, p=p, cam0=cam0, poses0=poses0, res=res, poses=poses)
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%s-mask%x-it%d" % c for c in CASES])
def test_device_equals_host(K, det, ref, i):
    r = ref[i]
    want = {0: (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED), 5: (A.CK_CALIB_MAXIT,)}.get(i, (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED, A.CK_CALIB_MAXIT))
    assert r["res"]["status"] in want and r["res"]["iters"] >= 3, (int(r["res"]["status"]), int(r["res"]["iters"]))
    res, poses = K.refine_batch(det, r["p"], [r["frames"]], [r["cam0"]], [r["poses0"]])
    print(CASES[i], "status", int(res[0]["status"]), "iters", int(res[0]["iters"]), "rms %.6f" % res[0]["rms"])
    assert res[0].tobytes() == r["res"].tobytes()
    assert poses[0].tobytes() == r["poses"].tobytes()
    res2, poses2 = K.calibrate_batch(det, r["p"], [r["frames"]])              # init + refine in one call: the same bytes
    assert res2[0].tobytes() == r["res"].tobytes() and poses2[0].tobytes() == r["poses"].tobytes()


def test_batch_composition(K, det, ref):
    idx = [0, 1, 4]                                    # the three shapes at mask 0, 100 iterations: one parameter set per call
    more = []
    for shape, seed in (("F4", 71), ("F3", 72)):
        frames = _frames(SHAPES[shape], seed)
        p = K.params(W, H)
        cam0, poses0, _ = K.calib_init(p, frames)
        res, poses = K.refine_host(p, frames, cam0, poses0)
        more.append(dict(frames=frames, p=p, cam0=cam0, poses0=poses0, res=res, poses=poses))
    five = [ref[i] for i in idx] + more
    p = K.params(W, H)
    for order in (range(5), (3, 0, 4, 2, 1)):
        sel = [five[j] for j in order]
        res, poses = K.refine_batch(det, p, [s["frames"] for s in sel], [s["cam0"] for s in sel], [s["poses0"] for s in sel])
        for s, r, P in zip(sel, res, poses):
            assert r.tobytes() == s["res"].tobytes() and P.tobytes() == s["poses"].tobytes()
    # a problem without a usable start in the middle: reported, its neighbours' bytes as before
    bad = dict(five[1], cam0=np.r_[0.0, five[1]["cam0"][1:]])
    sel = [five[0], five[3], bad, five[2], five[4]]
    res, poses = K.refine_batch(det, p, [s["frames"] for s in sel], [s["cam0"] for s in sel], [s["poses0"] for s in sel])
    for j, (s, r, P) in enumerate(zip(sel, res, poses)):
        if j == 2:
            want, wp = K.refine_host(p, s["frames"], s["cam0"], s["poses0"])
            assert r["status"] == A.CK_CALIB_DEGENERATE and r.tobytes() == want.tobytes() and P.tobytes() == wp.tobytes() == s["poses0"].tobytes()
        else:
            assert r.tobytes() == s["res"].tobytes() and P.tobytes() == s["poses"].tobytes()
    # ... and through ck_calibrate_batch: fronto-parallel frames have no start
    XY = N.board_points()
    k = N.cameras()["cam1_1600x1304"][0]
    flat = []
    for j, a in enumerate((0.0, 0.7, 1.9)):
        R = N.rodrigues(np.array([0, 0, a]))
        flat.append((XY, N.project(k, R, np.array([0.01 * j, 0.0, 1.0 + 0.1 * j]) - R[:, :2] @ XY.mean(0), XY)))
    res, poses = K.calibrate_batch(det, p, [five[0]["frames"], flat, five[2]["frames"]])
    assert res[1]["status"] == A.CK_CALIB_DEGENERATE and not res[1]["cam"].any() and not poses[1].any() and res[1]["n_points"] == 432
    assert res[0].tobytes() == five[0]["res"].tobytes() and res[2].tobytes() == five[2]["res"].tobytes()
    assert poses[0].tobytes() == five[0]["poses"].tobytes() and poses[2].tobytes() == five[2]["poses"].tobytes()


def test_two_runs_return_the_same_bytes(K, det, ref):
    sel = [ref[4], ref[1], ref[0]]
    p = K.params(W, H)
    runs = [K.refine_batch(det, p, [s["frames"] for s in sel], [s["cam0"] for s in sel], [s["poses0"] for s in sel]) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][1], runs[1][1]))


def test_misuse_on_the_device(K, det, ref):
    """The refusals of ck_calib_check through the device entry points, each followed by nothing worse than its code; a valid call after
    them all returns the right bytes."""
    from chalkydri_amd.detector import _bind
    from chalkydri_amd._lib import lib
    L = _bind(lib())
    r = ref[1]
    pk = K.Packed([r["frames"]])
    cams = (A.OpenCV5 * 1)(K._cam(r["cam0"]))
    res, poses = np.zeros(1, K.RESULT_DTYPE), np.zeros((4, 12))
    rp = C.cast(res.ctypes.data, C.POINTER(A.CalibResult))

    def both(p=None, h=det._h, prob=pk.prob, n=1, args=None, cams=cams, p0=r["poses0"].ctypes.data, rp=rp, out=poses.ctypes.data):
        p = C.byref(p or K.params(W, H))
        args = args or pk.args()
        a = L.ck_calib_refine_batch(h, p, prob, n, *args, cams, p0, rp, out)
        b = L.ck_calibrate_batch(h, p, prob, n, *args, rp, out)
        assert a == b or cams is None or p0 is None, (a, b)
        return a

    assert both(h=None) == A.CK_EINVAL and both(prob=None) == A.CK_EINVAL and both(rp=None) == A.CK_EINVAL and both(out=None) == A.CK_EINVAL
    assert L.ck_calib_refine_batch(det._h, C.byref(K.params(W, H)), pk.prob, 1, *pk.args(), None, r["poses0"].ctypes.data, rp, poses.ctypes.data) == A.CK_EINVAL
    assert L.ck_calib_refine_batch(det._h, C.byref(K.params(W, H)), pk.prob, 1, *pk.args(), cams, None, rp, poses.ctypes.data) == A.CK_EINVAL
    assert both(n=-1) == A.CK_EINVAL and both(n=0) == A.CK_OK
    for kw in ({"max_iters": 0}, {"max_iters": 10001}, {"min_frames": 5}, {"min_points_per_frame": 25}):
        assert both(p=K.params(W, H, **kw)) == A.CK_EINVAL, kw
    assert both(p=K.params(15, H)) == A.CK_EINVAL and both(p=K.params(W, 8)) == A.CK_EINVAL
    b, u, s, npts, nst, nfr = pk.args()
    bad_s = pk.frame_start.copy()
    bad_s[2] = bad_s[1] - 1
    assert both(args=(b, u, bad_s.ctypes.data, npts, nst, nfr)) == A.CK_EINVAL          # not monotone
    nan = pk.image_uv.copy()
    nan[30, 0] = np.nan
    assert both(args=(b, nan.ctypes.data, s, npts, nst, nfr)) == A.CK_EINVAL
    assert both(args=(None, u, s, npts, nst, nfr)) == A.CK_EINVAL and both(args=(b, u, s, npts - 1, nst, nfr)) == A.CK_EINVAL
    assert both(args=(b, u, s, npts, nst - 1, nfr)) == A.CK_EINVAL and both(args=(b, u, s, npts, nst, nfr - 1)) == A.CK_EINVAL
    assert both(prob=(A.CalibProblem * 1)(A.CalibProblem(A.CK_CALIB_MAX_FRAMES + 1, 0, 0, 0))) == A.CK_ECAPACITY
    big = np.zeros((A.CK_CALIB_MAX_POINTS + 1 + 48, 2))
    bs = np.array([0, A.CK_CALIB_MAX_POINTS + 1, A.CK_CALIB_MAX_POINTS + 25, A.CK_CALIB_MAX_POINTS + 49], np.int32)
    assert both(prob=(A.CalibProblem * 1)(A.CalibProblem(3, 0, 0, 0)), args=(big.ctypes.data, big.ctypes.data, bs.ctypes.data, len(big), 4, 3)) == A.CK_ECAPACITY
    got, P = K.refine_batch(det, r["p"], [r["frames"]], [r["cam0"]], [r["poses0"]])
    assert got[0].tobytes() == r["res"].tobytes() and P[0].tobytes() == r["poses"].tobytes()
    assert len(det.detect_batch(np.zeros((1, 480, 640), np.uint8))[0]) == 0                # the handle still detects


def test_end_to_end_from_rendered_frames(K, built, tmp_path):
    """The 6x6 board drawn under 4 poses of a known pinhole camera at 1280x800 -> Calibrator.process -> calibrate with the distortion
    frozen.  The corner order of the observations is right when the reprojection rms is that of the detector's corner noise: the bound
    is 1.5 times the rms scipy reaches on the same observations (both printed).  The device result equals the host twin's on these
    observations, the dict goes into AprilTags as it is, and the C++ Calibrator keeps the same 4 frames.
    Measured on an MI355X: 144 corners per frame, rms 0.2048 px, scipy 0.2048 px, bound 0.3072 px."""
    from chalkydri_amd import synth
    from chalkydri_amd.apriltags import AprilTags
    from chalkydri_amd.detector import AprilTagDetector
    w, h = 1280, 800
    Kc = np.array([[920.0, 0, 652.0], [0, 915.0, 391.0], [0, 0, 1]])
    board = K.Board.default_6x6()
    ctr = board.points().mean(0)
    s = board.tag_size / 2
    frames = np.zeros((4, h, w), np.uint8)
    for f, (tilt, axis, spin, z) in enumerate(((0.45, 0.3, 0.10, 1.05), (0.40, 1.9, -0.15, 1.10), (0.50, 3.6, 0.05, 1.15), (0.35, 5.0, 0.20, 1.20))):
        R = N.rodrigues(tilt * np.array([np.cos(axis), np.sin(axis), 0.0])) @ N.rodrigues(np.array([0, 0, spin]))
        t = np.array([0.01 * f, -0.01 * f, z]) - R[:, :2] @ ctr
        Hb = Kc @ np.column_stack([R[:, 0], R[:, 1], t])
        tags = []
        for tid in board.ids():
            c = board.tag_center(tid)
            Ht = Hb @ np.array([[s, 0, c[0]], [0, s, c[1]], [0, 0, 1.0]])
            tags.append((0, tid, Ht))
            px = (Ht @ np.array([[-1, 1, 1], [1, 1, 1], [1, -1, 1], [-1, -1, 1.0]]).T).T
            px = px[:, :2] / px[:, 2:]
            assert min(np.linalg.norm(px[i] - px[(i + 1) % 4]) for i in range(4)) >= 40      # every tag at least 40 px on a side
            assert px.min() > 20 and px[:, 0].max() < w - 20 and px[:, 1].max() < h - 20
        frames[f] = synth.render_scene(synth.frame_seed(9, f), w, h, tags)[0]
    det = AprilTagDetector(w, h, max_batch=4)
    cal = K.Calibrator(det, board)
    assert cal.process(frames) == 4
    obs = cal.observations()
    assert all(len(b) >= 24 for b, _ in obs)
    print("corners per frame:", [len(b) for b, _ in obs])
    p = K.params(w, h, fixed_mask=K.FIX_DISTORTION)
    cam0, poses0, st = K.calib_init(p, obs)
    assert st == A.CK_CALIB_CONVERGED
    _, ref_rms, _ = N.solve(obs, cam0, poses0, fixed_mask=K.FIX_DISTORTION)
    out = cal.calibrate(fixed_mask=K.FIX_DISTORTION, leave_out=3, seed=1)
    assert out is not None
    calib, report = out
    print("rms %.4f px, scipy on the same observations %.4f px, bound %.4f" % (report["rms"], ref_rms, 1.5 * ref_rms), calib["OpenCVModel5"], report["std"])
    assert report["rms"] <= 1.5 * ref_rms and report["status"] in ("converged", "stalled")
    assert len(report["per_frame_rms"]) == 4 and max(report["per_frame_rms"]) <= 3 * ref_rms and report["n_subsets"] >= 2
    assert all(np.isfinite(v) and v < 20 for v in report["std"].values()) and report["std"]["k1"] == 0
    m = calib["OpenCVModel5"]
    assert abs(m["fx"] - 920) < 10 and abs(m["fy"] - 915) < 10 and abs(m["cx"] - 652) < 10 and abs(m["cy"] - 391) < 10 and m["k1"] == 0 and m["k3"] == 0
    want, wposes = K.refine_host(p, obs, cam0, poses0)
    assert np.array([m[n] for n in K.PARAM_NAMES]).tobytes() == want["cam"].tobytes() and report["poses"].tobytes() == wposes.tobytes()
    assert report["rms"] == want["rms"] and report["iters"] == want["iters"]
    cal.clear()
    assert cal.process(frames[:1]) == 1 and cal.calibrate() is None                      # fewer than min_frames frames: None
    det.close()
    task = AprilTags(w, h, {"tags": []}, calib, {"roll": 0, "pitch": 0, "yaw": 0, "x": 0, "y": 0, "z": 0})
    assert (task.cam.fx, task.cam.cy, task.cam.k2) == (m["fx"], m["cy"], 0.0)
    task.detector.close()
    (tmp_path / "frames.bin").write_bytes(np.int32(4).tobytes() + frames.tobytes())
    r = subprocess.run([os.path.join(ROOT, "chalkydri_amd", "lib", "calib_demo"), "frames", str(w), str(h), str(K.FIX_DISTORTION), str(tmp_path / "frames.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "KEPT 4" and r.stdout.splitlines()[1].startswith("OK"), (r.stdout, r.stderr)
    assert float(r.stdout.splitlines()[1].split()[1]) == m["fx"]
