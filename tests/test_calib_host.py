"""The host half of the camera calibration: ck_calib_init, ck_calib_refine_host (the bitwise specification of the device
solver), ck_calib_jacobian and ck_calib_check, against the truth and against tests/np_calib.py (numpy + scipy, Rodrigues poses, numeric
Jacobians: no code shared with the library).  No GPU.

Inputs: the reference's two 1600x1304 cameras (tests/golden/calib_cameras.json), F in {4, 8} frames of the 6x6 board, noise 0 and 0.1 px,
seeds 0..4 of np_calib.make_case: 40 cases.  Bounds, each 100 times the reference's own largest distance on these 40 cases (two optimisers
stop at different points of a flat valley), measured once and fixed here:
  noise-free   scipy trf to the truth: 5.46e-12 at most over the nine parameters -> BOUND_TRUTH = 5.5e-10 (the library: 3.4e-10 at most)
  0.1 px       scipy trf to scipy lm (200000 evaluations allowed) at the same minimum: 1.21e-4 at most -> BOUND_MINIMUM = 1.3e-2
               (the library to trf: 2.4e-6 at most)
  Jacobian     central differences at relative step 1e-5 against step 5e-6, per column relative to the column's largest entry: 2.7e-7 at
               most -> BOUND_JACOBIAN = 2.7e-5 (the analytic Jacobian to the finer differences: 2.3e-7 at most)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_calib as N  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

BOUND_TRUTH, BOUND_MINIMUM, BOUND_JACOBIAN = 5.5e-10, 1.3e-2, 2.7e-5
CAMS = ("cam1_1600x1304", "cam0_1600x1304")
DIST = A.CK_CALIB_FIX_DISTORTION


@pytest.fixture(scope="module")
def K(built):
    from chalkydri_amd import calibration
    return calibration


def _solve(K, frames, w, h, **kw):
    p = K.params(w, h, **kw)
    cam0, poses0, st = K.calib_init(p, frames)
    assert st == A.CK_CALIB_CONVERGED
    res, poses = K.refine_host(p, frames, cam0, poses0)
    return cam0, poses0, res, poses


@pytest.mark.parametrize("F", (4, 8))
@pytest.mark.parametrize("name", CAMS)
def test_noise_free_reaches_the_truth(K, name, F):
    k, w, h = N.cameras()[name]
    for seed in range(5):
        frames, truth = N.make_case(k, w, h, F, 0.0, seed)
        cam0, poses0, res, poses = _solve(K, frames, w, h)
        err = float(np.max(np.abs(res["cam"] - k)))
        print(name, F, seed, "start fx %.0f" % cam0[0], "iters", int(res["iters"]), "rms %.3g" % res["rms"], "err %.3g" % err)
        assert res["status"] == A.CK_CALIB_CONVERGED, (seed, int(res["status"]))
        assert err <= BOUND_TRUTH, (seed, err)
        assert res["n_frames"] == F and res["n_points"] == sum(len(f[0]) for f in frames) and res["cost"] <= res["cost0"]
        for P, (R, t) in zip(poses, truth):
            assert np.max(np.abs(P[:9].reshape(3, 3) - R)) < 1e-9 and np.max(np.abs(P[9:] - t)) < 1e-9


@pytest.mark.parametrize("F", (4, 8))
@pytest.mark.parametrize("name", CAMS)
def test_noisy_reaches_scipys_minimum(K, name, F):
    k, w, h = N.cameras()[name]
    for seed in range(5):
        frames, _ = N.make_case(k, w, h, F, 0.1, seed)
        cam0, poses0, res, _ = _solve(K, frames, w, h)
        ks, rms, _ = N.solve(frames, cam0, poses0)
        err = float(np.max(np.abs(res["cam"] - ks)))
        print(name, F, seed, "status", int(res["status"]), "iters", int(res["iters"]), "rms %.6f scipy %.6f" % (res["rms"], rms), "err %.3g" % err)
        assert res["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED), (seed, int(res["status"]))
        assert err <= BOUND_MINIMUM, (seed, err)
        assert abs(res["rms"] - rms) <= 1e-9 and res["rms"] == np.sqrt(res["cost"] / res["n_points"])


def _cayley(w):
    Kx = 0.5 * np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.linalg.solve(np.eye(3) - Kx, np.eye(3) + Kx)


def _resid(k, R, t, XY, uv, d):
    return N.project(k + d[:9], R @ _cayley(d[9:12]), t + d[12:], XY) - uv


def _central(k, R, t, XY, uv, h):
    J = np.zeros((len(XY), 2, 15))
    for j in range(15):
        d = np.zeros(15)
        d[j] = s = h * (abs(k[j]) if j < 9 else 1.0)
        J[:, :, j] = (_resid(k, R, t, XY, uv, d) - _resid(k, R, t, XY, uv, -d)) / (2 * s)
    return J


def test_analytic_jacobian_against_central_differences(K):
    worst = 0.0
    for name in CAMS:
        k, w, h = N.cameras()[name]
        for seed in range(4):
            frames, poses = N.make_case(k, w, h, 4, 0.1, 100 + seed)
            for (XY, uv), (R, t) in zip(frames, poses):
                r, J = K.jacobian(k, np.concatenate([R.ravel(), t]), XY, uv)
                assert np.max(np.abs(r - _resid(k, R, t, XY, uv, np.zeros(15)))) < 1e-9
                rel = np.max(np.max(np.abs(J - _central(k, R, t, XY, uv, 5e-6)), axis=(0, 1)) / np.max(np.abs(J), axis=(0, 1)))
                worst = max(worst, float(rel))
    print("analytic against central differences: %.3g" % worst)
    assert worst <= BOUND_JACOBIAN
    k, w, h = N.cameras()[CAMS[0]]
    (XY, uv), (R, t) = [x[0] for x in N.make_case(k, w, h, 3, 0.0, 7)]
    _, J = K.jacobian(k, np.concatenate([R.ravel(), t]), XY, uv, fixed_mask=0x111)
    assert not J[:, :, [0, 4, 8]].any() and J[:, :, [1, 2, 3, 5, 6, 7]].any(axis=(0, 1)).all()


def test_fixed_mask(K):
    k, w, h = N.cameras()[CAMS[0]]
    frames, _ = N.make_case(k, w, h, 4, 0.1, 3)
    p = K.params(w, h)
    cam0, poses0, _ = K.calib_init(p, frames)
    start = cam0.copy()
    start[4:] = [-0.03, 0.001, 0.0005, -0.0002, 0.01]
    for mask in (DIST, A.CK_CALIB_FIX_FOCAL, 0x1FF, 0x00C):
        res, _ = K.refine_host(K.params(w, h, fixed_mask=mask), frames, start, poses0)
        for i in range(9):
            if (mask >> i) & 1:
                assert res["cam"][i].tobytes() == start[i].tobytes(), (mask, i)     # frozen: bit-unchanged
            else:
                assert res["cam"][i] != start[i], (mask, i)
        assert res["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED) and res["cost"] < res["cost0"]
    # a pinhole camera with all distortion frozen at zero: the truth
    kp = k.copy()
    kp[4:] = 0
    for F in (4, 8):
        frames, _ = N.make_case(kp, w, h, F, 0.0, 11)
        _, _, res, _ = _solve(K, frames, w, h, fixed_mask=DIST)
        assert res["status"] == A.CK_CALIB_CONVERGED and np.max(np.abs(res["cam"] - kp)) <= BOUND_TRUTH
        assert not res["cam"][4:].any()


def test_degenerate_inputs_are_reported_not_solved(K):
    k, w, h = N.cameras()[CAMS[0]]
    XY = N.board_points()
    ctr = XY.mean(0)

    def frame(R, t, sel=slice(None)):
        return XY[sel], N.project(k, R, t, XY[sel])
    # fronto-parallel frames only: the orthogonality equations say 0 = 0
    flat = [frame(N.rodrigues(np.array([0, 0, a])), np.array([0.02 * i, -0.01 * i, 0.7 + 0.1 * i]) - N.rodrigues(np.array([0, 0, a]))[:, :2] @ ctr)
            for i, a in enumerate((0.0, 0.7, 1.9, 3.0))]
    # collinear points: one row of corners per frame, no homography
    row = [frame(N.rodrigues(np.array([0.3, 0.1 * i, 0.2])), np.array([-0.3, -0.1, 0.8])) for i in range(4)]
    row = [(b[np.isclose(b[:, 1], 0.088)][:24], u[np.isclose(b[:, 1], 0.088)][:24]) for b, u in row]
    assert all(len(b) >= 6 for b, _ in row)
    for frames, mp in ((flat, 24), (row, 6)):
        p = K.params(w, h, min_points_per_frame=mp)
        cam0, poses0, st = K.calib_init(p, frames)
        assert np.isfinite(cam0).all() and np.isfinite(poses0).all()
        res, poses = K.refine_host(p, frames, cam0, poses0)
        assert st == A.CK_CALIB_DEGENERATE and res["status"] == A.CK_CALIB_DEGENERATE
        assert np.isfinite(res["cam"]).all() and np.isfinite(poses).all() and np.isfinite([res["rms"], res["cost0"], res["cost"]]).all()
        assert res["iters"] == 0 and res["rms"] == 0 and res["cam"].tobytes() == cam0.tobytes()
    # a start the solver cannot evaluate, or that sits where nothing can be gained: reported, finite
    frames, _ = N.make_case(k, w, h, 4, 0.0, 1)
    p = K.params(w, h)
    cam0, poses0, _ = K.calib_init(p, frames)
    for bad in (np.r_[0.0, cam0[1:]], np.r_[cam0[:4], np.nan, cam0[5:]]):
        res, poses = K.refine_host(p, frames, bad, poses0)
        assert res["status"] == A.CK_CALIB_DEGENERATE and res["cam"].tobytes() == bad.tobytes() and poses.tobytes() == poses0.tobytes()
    behind = poses0.copy()
    behind[0, 9:] = -behind[0, :9].reshape(3, 3)[:, :2] @ frames[0][0][0]      # the first point of frame 0 at the camera centre: z = 0
    res, poses = K.refine_host(p, frames, cam0, behind)
    assert res["status"] == A.CK_CALIB_DEGENERATE and res["cost0"] == 0 and poses.tobytes() == behind.tobytes()
    res, _ = K.refine_host(K.params(w, h, fixed_mask=0x1FF), flat, np.r_[k[:4], np.zeros(5)], poses0)   # wrong model, nothing free but poses
    assert res["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED, A.CK_CALIB_MAXIT) and np.isfinite(res["cam"]).all() and np.isfinite(res["rms"])


def test_the_1280x720_camera_is_reported_honestly(K):
    """Not an acceptance input: the scipy prototype of this solver did not converge on 7 of its 20 cases.  What the library does on
    them (DESIGN.md §4j has the table): every run ends with a status, finite numbers, and a cost not above its start's."""
    k, w, h = N.cameras()["cam2_1280x720"]
    seen = {}
    for F in (4, 8):
        for noise in (0.0, 0.1):
            for seed in range(5):
                frames, _ = N.make_case(k, w, h, F, noise, seed)
                p = K.params(w, h)
                cam0, poses0, st = K.calib_init(p, frames)
                res, poses = K.refine_host(p, frames, cam0, poses0)
                assert (st == A.CK_CALIB_DEGENERATE) == (res["status"] == A.CK_CALIB_DEGENERATE)
                assert np.isfinite(res["cam"]).all() and np.isfinite(poses).all() and np.isfinite(res["rms"]) and res["cost"] <= res["cost0"]
                if noise == 0 and res["status"] == A.CK_CALIB_CONVERGED:
                    assert np.max(np.abs(res["cam"] - k)) < 1e-6
                seen[int(res["status"])] = seen.get(int(res["status"]), 0) + 1
    print("statuses on the 1280x720 camera:", seen)


def test_refusals(K):
    from chalkydri_amd._lib import lib
    from chalkydri_amd.detector import _bind
    L = _bind(lib())
    k, w, h = N.cameras()[CAMS[0]]
    frames, _ = N.make_case(k, w, h, 4, 0.0, 2)
    pk = K.Packed([frames])

    def rc(p=None, prob=None, b=None, u=None, s=None, npts=None, nst=None, nfr=None):
        p = p or K.params(w, h)
        prob = pk.prob if prob is None else prob
        b, u, s = (pk.board_xy if b is None else b), (pk.image_uv if u is None else u), (pk.frame_start if s is None else s)
        ptr = lambda a: None if isinstance(a, int) else a.ctypes.data
        args = (ptr(b), ptr(u), ptr(s), pk.n_points if npts is None else npts, pk.n_starts if nst is None else nst, pk.n_frames if nfr is None else nfr)
        got = L.ck_calib_check(C.byref(p), prob, 1, *args)
        cam, poses, st, res = A.OpenCV5(), np.zeros((8, 12)), C.c_int32(0), A.CalibResult()
        if got != A.CK_OK:   # every entry point refuses what the check refuses
            assert L.ck_calib_init(C.byref(p), prob, *args, C.byref(cam), poses.ctypes.data, C.byref(st)) == got
            assert L.ck_calib_refine_host(C.byref(p), prob, *args, C.byref(cam), poses.ctypes.data, C.byref(res), poses.ctypes.data) == got
        return got

    def prob(**kw):
        q = A.CalibProblem(4, 0, 0, 0)
        for n, v in kw.items():
            setattr(q, n, v)
        return (A.CalibProblem * 1)(q)

    assert rc() == A.CK_OK
    for kw in ({"max_iters": 0}, {"max_iters": 10001}, {"min_points_per_frame": 3}, {"min_frames": 0}, {"min_frames": 5}, {"min_points_per_frame": 145}):
        assert rc(p=K.params(w, h, **kw)) == A.CK_EINVAL, kw
    assert rc(p=K.params(15, h)) == A.CK_EINVAL and rc(p=K.params(w, 15)) == A.CK_EINVAL and rc(p=K.params(16, 16)) == A.CK_OK
    assert rc(p=K.params(w, h, max_iters=1)) == A.CK_OK and rc(p=K.params(w, h, max_iters=10000)) == A.CK_OK
    for null in ("b", "u", "s"):
        assert rc(**{null: 0}) == A.CK_EINVAL
    assert L.ck_calib_check(None, pk.prob, 1, *pk.args()) == A.CK_EINVAL and L.ck_calib_check(C.byref(K.params(w, h)), None, 1, *pk.args()) == A.CK_EINVAL
    assert L.ck_calib_check(C.byref(K.params(w, h)), pk.prob, -1, *pk.args()) == A.CK_EINVAL
    s = pk.frame_start.copy()
    s[2] = s[1] - 1
    assert rc(s=s) == A.CK_EINVAL                                                   # not monotone
    s = pk.frame_start.copy()
    s[2] = s[1] + 23
    assert rc(s=s) == A.CK_EINVAL                                                   # a frame below min_points_per_frame
    for arr in ("b", "u"):
        for v in (np.nan, np.inf):
            a = (pk.board_xy if arr == "b" else pk.image_uv).copy()
            a[17, 1] = v
            assert rc(**{arr: a}) == A.CK_EINVAL
    assert rc(npts=pk.n_points - 1) == A.CK_EINVAL and rc(nst=4) == A.CK_EINVAL and rc(nfr=3) == A.CK_EINVAL
    assert rc(prob=prob(start_offset=1)) == A.CK_EINVAL and rc(prob=prob(point_offset=1)) == A.CK_EINVAL and rc(prob=prob(pose_offset=-1)) == A.CK_EINVAL
    assert rc(prob=prob(n_frames=2)) == A.CK_EINVAL
    assert rc(prob=prob(n_frames=A.CK_CALIB_MAX_FRAMES + 1)) == A.CK_ECAPACITY
    big = np.zeros((A.CK_CALIB_MAX_POINTS + 1 + 3 * 24, 2))
    s = np.array([0, A.CK_CALIB_MAX_POINTS + 1, A.CK_CALIB_MAX_POINTS + 25, A.CK_CALIB_MAX_POINTS + 49, A.CK_CALIB_MAX_POINTS + 73], np.int32)
    assert rc(b=big, u=big, s=s, npts=len(big)) == A.CK_ECAPACITY
    s[1] -= 1
    assert rc(b=big, u=big, s=s, npts=len(big)) == A.CK_OK
    cam, poses, res = A.OpenCV5(), np.zeros((4, 12)), A.CalibResult()
    p = K.params(w, h)
    assert L.ck_calib_init(C.byref(p), pk.prob, *pk.args(), None, poses.ctypes.data, C.byref(C.c_int32())) == A.CK_EINVAL
    assert L.ck_calib_refine_host(C.byref(p), pk.prob, *pk.args(), C.byref(cam), poses.ctypes.data, None, poses.ctypes.data) == A.CK_EINVAL
    assert L.ck_calib_jacobian(None, poses.ctypes.data, pk.board_xy.ctypes.data, pk.image_uv.ctypes.data, 1, 0, poses.ctypes.data, poses.ctypes.data) == A.CK_EINVAL


def test_board_and_defaults(K):
    b = K.Board.default_6x6()
    assert (b.rows, b.cols, b.tag_size, b.tag_spacing, b.first_id) == (6, 6, 0.088, 0.3, 0)
    assert np.array_equal(b.points(), N.board_points())                 # the restatement's board
    c = K.Board(2, 3, 0.1, 0.5, first_id=10).tag_corners(14)            # row 1, column 1
    assert np.allclose(c, np.array([0.15, 0.15]) + [[0, 0.1], [0.1, 0.1], [0.1, 0], [0, 0]])
    with pytest.raises(KeyError):
        b.tag_corners(36)
    p = K.params(640, 480)
    assert (p.width, p.height, p.fixed_mask, p.max_iters, p.min_points_per_frame, p.min_frames) == (640, 480, 0, 100, 24, 3)
    import chalkydri_amd
    assert chalkydri_amd.Calibrator is K.Calibrator and chalkydri_amd.Board is K.Board
