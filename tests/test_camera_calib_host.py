"""The host half of the EUCM / UCM calibration: ck_camera_calib_init's ladder of starts, ck_camera_calib_refine_host (the
bitwise specification of the device solver) and ck_camera_calib_jacobian, against the truth and against tests/np_camera_calib.py (the
numpy restatement of the model + scipy, Rodrigues poses, numeric Jacobians: no code shared with the library).  No GPU.

Inputs: the three lenses of tests/np_camera.py on 1280 x 800, F in {4, 8} frames of np_calib.board_points(), noise 0 and 0.1 px, seeds
0..4 of np_camera_calib.make_case: 60 captures, each solved from the six starts; the winner is the lowest finite final cost, lowest
index on ties (ck_camera_calibrate_batch's rule).  Bounds, from the reference's own error on these captures, measured once and fixed:
  noise-free   scipy trf started AT THE TRUTH leaves at most 7.96e-13 over the six parameters -> BOUND_TRUTH = 10 x that = 8e-12
               (the library's winner: 2.2e-12 at most)
  0.1 px       rms: within 1e-9 px of scipy's minimum from the winner's own start, test_noisy_reaches_scipys_minimum's bound (measured:
               1.1e-14 at most).  Parameters: two scipy runs of one capture, from the winner's start and from the truth, differ by at
               most 1.03e-6 -> BOUND_MINIMUM = 10 x that = 1.03e-5 (the library to scipy from the same start: 7.0e-7 at most)
  Jacobian     test_calib_host.py's relative bound for the analytic Jacobian against central differences, BOUND_JACOBIAN = 2.7e-5
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_calib as N  # noqa: E402
import np_camera as NC  # noqa: E402
import np_camera_calib as M  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

BOUND_TRUTH, BOUND_MINIMUM, BOUND_JACOBIAN = 8e-12, 1.03e-5, 2.7e-5
LENSES = ("eucm_wide", "ucm", "eucm_mild")


def _model(name):
    return "UCM" if name == "ucm" else "EUCM"


@pytest.fixture(scope="module")
def K(built):
    from chalkydri_amd import calibration
    return calibration


def solve_all_starts(K, model, p, frames):
    """Every start of the ladder through the host twin, and the winner by ck_camera_calibrate_batch's rule: (index, list of
    (result, poses, k0, poses0))."""
    outs = []
    for s in range(A.CK_CAMCAL_STARTS):
        k0, p0, st = K.camera_calib_init(model, p, frames, s)
        res, poses = K.camera_refine_host(model, p, frames, k0, p0)
        assert (st == A.CK_CALIB_DEGENERATE) <= (res["status"] == A.CK_CALIB_DEGENERATE)
        outs.append((res, poses, k0, p0))
    ok = [i for i, o in enumerate(outs) if o[0]["status"] != A.CK_CALIB_DEGENERATE and np.isfinite(o[0]["cost"])]
    return (min(ok, key=lambda i: (float(outs[i][0]["cost"]), i)) if ok else -1), outs


@pytest.mark.parametrize("F", (4, 8))
@pytest.mark.parametrize("name", LENSES)
def test_noise_free_best_start_reaches_the_truth(K, name, F):
    lens = np.array(NC.LENSES[name])
    for seed in range(5):
        frames, truth = M.make_case(tuple(lens), F, 0.0, seed)
        win, outs = solve_all_starts(K, _model(name), K.params(NC.W, NC.H), frames)
        res, poses = outs[win][:2]
        err = float(np.max(np.abs(res["cam"][:6] - lens)))
        print(name, F, seed, "winner", win, "iters", int(res["iters"]), "rms %.3g" % res["rms"], "err %.3g" % err,
              "finals", ["%.2g" % o[0]["rms"] for o in outs])
        assert res["status"] == A.CK_CALIB_CONVERGED, (seed, int(res["status"]))
        assert err <= BOUND_TRUTH, (seed, err)
        assert not res["cam"][6:].any() and res["model"] == (A.CK_CAMERA_UCM if name == "ucm" else A.CK_CAMERA_EUCM)
        assert res["n_frames"] == F and res["n_points"] == sum(len(f[0]) for f in frames) and res["cost"] <= res["cost0"]
        for P, (R, t) in zip(poses, truth):
            assert np.max(np.abs(P[:9].reshape(3, 3) - R)) < 1e-9 and np.max(np.abs(P[9:] - t)) < 1e-9


@pytest.mark.parametrize("F", (4, 8))
@pytest.mark.parametrize("name", LENSES)
def test_noisy_winner_reaches_scipys_minimum(K, name, F):
    lens = np.array(NC.LENSES[name])
    for seed in range(5):
        frames, _ = M.make_case(tuple(lens), F, 0.1, seed)
        win, outs = solve_all_starts(K, _model(name), K.params(NC.W, NC.H), frames)
        res, _, k0, p0 = outs[win]
        ks, rms, _ = M.solve(frames, k0, p0, ucm=name == "ucm")
        err = float(np.max(np.abs(res["cam"][:6] - ks)))
        print(name, F, seed, "winner", win, "status", int(res["status"]), "iters", int(res["iters"]), "rms %.6f scipy %.6f" % (res["rms"], rms),
              "err %.3g" % err)
        assert res["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED), (seed, int(res["status"]))
        assert abs(res["rms"] - rms) <= 1e-9 and res["rms"] == np.sqrt(res["cost"] / res["n_points"])
        assert err <= BOUND_MINIMUM, (seed, err)


def _cayley(w):
    Kx = 0.5 * np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.linalg.solve(np.eye(3) - Kx, np.eye(3) + Kx)


def _resid(k, R, t, XY, uv, d):
    return M.project(tuple(k + d[:6]), R @ _cayley(d[9:12]), t + d[12:], XY)[0] - uv


def _central(k, R, t, XY, uv, h, cols):
    J = np.zeros((len(XY), 2, 15))
    for j in cols:
        d = np.zeros(15)
        d[j] = s = h * (abs(k[j]) if j < 6 else 1.0)
        J[:, :, j] = (_resid(k, R, t, XY, uv, d) - _resid(k, R, t, XY, uv, -d)) / (2 * s)
    return J


@pytest.mark.parametrize("name", LENSES)
def test_analytic_jacobian_against_central_differences(K, name):
    """Columns fx fy cx cy alpha beta, then rotation and translation increments, in the manner and with the bound of test_calib_host.py's
    test of the same name; slots 6..8 are zero columns, and so is UCM's beta."""
    k = np.array(NC.LENSES[name])
    cols = [c for c in range(15) if c not in (6, 7, 8) and not (name == "ucm" and c == 5)]
    worst = 0.0
    for seed in range(4):
        frames, poses = M.make_case(tuple(k), 4, 0.1, 100 + seed)
        for (XY, uv), (R, t) in zip(frames, poses):
            r, J = K.camera_jacobian(_model(name), k, M.pose12(R, t), XY, uv)
            assert np.max(np.abs(r - _resid(k, R, t, XY, uv, np.zeros(15)))) < 1e-9
            Jc = _central(k, R, t, XY, uv, 5e-6, cols)
            rel = np.max(np.max(np.abs(J - Jc)[:, :, cols], axis=(0, 1)) / np.max(np.abs(J)[:, :, cols], axis=(0, 1)))
            worst = max(worst, float(rel))
            assert not J[:, :, [c for c in range(9) if c not in cols]].any()
    print(name, "analytic against central differences: %.3g" % worst)
    assert worst <= BOUND_JACOBIAN
    (XY, uv), (R, t) = [x[0] for x in M.make_case(tuple(k), 3, 0.0, 7)]
    _, J = K.camera_jacobian(_model(name), k, M.pose12(R, t), XY, uv, fixed_mask=0x11)
    assert not J[:, :, [0, 4]].any() and J[:, :, [1, 2, 3]].any(axis=(0, 1)).all()


def test_opencv5_through_the_camera_entry_points_is_byte_equal(K):
    """model = OPENCV5: start 0 (the only one), the Jacobian and the host refinement return the bytes of ck_calib_init,
    ck_calib_jacobian and ck_calib_refine_host."""
    k, w, h = N.cameras()["cam1_1600x1304"]
    for F, noise, mask in ((4, 0.1, 0), (3, 0.0, A.CK_CALIB_FIX_DISTORTION), (8, 0.1, 0x00C)):
        frames, poses = N.make_case(k, w, h, F, noise, 11)
        p = K.params(w, h, fixed_mask=mask)
        cam0, poses0, st = K.calib_init(p, frames)
        kc0, pc0, stc = K.camera_calib_init("OpenCVModel5", p, frames, 0)
        assert st == stc == A.CK_CALIB_CONVERGED and kc0.tobytes() == cam0.tobytes() and pc0.tobytes() == poses0.tobytes()
        (XY, uv), (R, t) = frames[0], poses[0]
        r, J = K.jacobian(k, M.pose12(R, t), XY, uv, mask)
        rc, Jc = K.camera_jacobian("OpenCVModel5", k, M.pose12(R, t), XY, uv, mask)
        assert r.tobytes() == rc.tobytes() and J.tobytes() == Jc.tobytes()
        start = cam0.copy()
        start[4:] = [-0.03, 0.001, 0.0005, -0.0002, 0.01]
        res, out = K.refine_host(p, frames, start, poses0)
        resc, outc = K.camera_refine_host("OpenCVModel5", p, frames, start, poses0)
        assert out.tobytes() == outc.tobytes() and resc["cam"].tobytes() == res["cam"].tobytes()
        for f in ("status", "iters", "n_frames", "n_points", "rms", "cost0", "cost"):
            assert resc[f].tobytes() == res[f].tobytes(), f
        assert (resc["model"], resc["start"], resc["n_starts"]) == (A.CK_CAMERA_OPENCV5, 0, 1)
    with pytest.raises(Exception):
        K.camera_calib_init("OpenCVModel5", p, frames, 1)                    # OpenCVModel5 has one start
    with pytest.raises(Exception):
        K.camera_calib_init("EUCM", p, frames, A.CK_CAMCAL_STARTS)
    with pytest.raises(Exception):
        K.camera_calib_init(3, p, frames, 0)                                 # an unknown model


def test_ladder_of_starts(K):
    """Start 0 has ck_calib_init's focal lengths, starts 1..5 fx = fy = {0.3, 0.45, 0.65, 1.0, 1.5} max(width, height); every start has
    the principal point at the image centre, alpha 0.5, beta 1 and poses in front of the camera."""
    frames, _ = M.make_case(NC.LENSES["eucm_mild"], 4, 0.1, 2)
    p = K.params(NC.W, NC.H)
    cam0, _, st0 = K.calib_init(p, frames)
    for s, c in enumerate((None, 0.3, 0.45, 0.65, 1.0, 1.5)):
        k0, poses0, st = K.camera_calib_init("EUCM", p, frames, s)
        assert st == A.CK_CALIB_CONVERGED and list(k0[2:]) == [(NC.W - 1) / 2, (NC.H - 1) / 2, 0.5, 1.0, 0, 0, 0]
        assert list(k0[:2]) == (list(cam0[:2]) if c is None else [c * NC.W] * 2)
        assert (poses0[:, 11] > 0).all() and np.isfinite(poses0).all()
        for P in poses0:
            R = P[:9].reshape(3, 3)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12


def test_fixed_mask_freezes_eucm_slots_bit_for_bit(K):
    lens = NC.LENSES["eucm_wide"]
    frames, _ = M.make_case(lens, 4, 0.1, 3)
    k0, poses0, _ = K.camera_calib_init("EUCM", K.params(NC.W, NC.H), frames, 2)
    start = k0.copy()
    start[4:6] = [0.58, 1.13]
    for mask in (1 << 5, 0x003, 0x03F, 0x00C, 1 << 4):
        res, _ = K.camera_refine_host("EUCM", K.params(NC.W, NC.H, fixed_mask=mask), frames, start, poses0)
        assert res["status"] != A.CK_CALIB_DEGENERATE and res["iters"] > 0
        for i in range(9):
            if (mask >> i) & 1 or i >= 6:
                assert res["cam"][i].tobytes() == start[i].tobytes(), (mask, i)     # frozen: bit-unchanged
            elif mask != 0x03F:
                assert res["cam"][i] != start[i], (mask, i)
    res, _ = K.camera_refine_host("UCM", K.params(NC.W, NC.H), frames, start, poses0)   # UCM: slot 5 is 1.0 whatever the start holds
    assert res["cam"][5] == 1.0 and res["model"] == A.CK_CAMERA_UCM


def test_a_step_out_of_the_model_is_rejected_not_clamped(K):
    """From alpha = 0.99 on a lens with alpha = 0.62 the first Gauss-Newton steps overshoot alpha's end of [0, 1] or lose observations
    behind the projection's cone: such a candidate's cost is NaN and the step is rejected (more damping), never clamped.  With one
    iteration allowed the parameters come back bit for bit; with a hundred, alpha has moved and never sat on a bound."""
    lens = NC.LENSES["eucm_wide"]
    frames, truth = M.make_case(lens, 4, 0.0, 1)
    poses0 = np.array([M.pose12(R, t) for R, t in truth])
    start = np.array(lens + (0, 0, 0), float)
    start[4] = 0.99
    # a candidate outside the model, by construction: the Jacobian's residual at alpha just past 1 is NaN
    r, _ = K.camera_jacobian("EUCM", np.array(lens[:4] + (1.0 + 1e-12, 1.08)), poses0[0], *frames[0])
    assert np.isnan(r).all()
    r, _ = K.camera_jacobian("EUCM", np.array(lens[:5] + (0.0,)), poses0[0], *frames[0])
    assert np.isnan(r).all()
    trail = []
    for iters in range(1, 13):
        res, _ = K.camera_refine_host("EUCM", K.params(NC.W, NC.H, max_iters=iters), frames, start, poses0)
        trail.append((float(res["cam"][4]), float(res["cost"])))
        assert 0.0 < res["cam"][4] < 1.0 and np.isfinite(res["cost"]) and res["cost"] <= res["cost0"]
    rejected = [i for i in range(1, len(trail)) if trail[i] == trail[i - 1]] + ([0] if trail[0][0] == 0.99 else [])
    print("alpha and cost by max_iters:", trail)
    assert rejected, "no step was rejected: the case does not exercise the rule"
    res, _ = K.camera_refine_host("EUCM", K.params(NC.W, NC.H), frames, start, poses0)
    assert res["status"] == A.CK_CALIB_CONVERGED and abs(res["cam"][4] - 0.62) < 1e-9
    # a start outside the model cannot be evaluated
    bad = start.copy()
    bad[4] = 1.2
    res, out = K.camera_refine_host("EUCM", K.params(NC.W, NC.H), frames, bad, poses0)
    assert res["status"] == A.CK_CALIB_DEGENERATE and res["iters"] == 0 and res["cam"].tobytes() == bad.tobytes() and out.tobytes() == poses0.tobytes()


NEAR_PINHOLE = (600.0, 600.0, 639.5, 399.5, 0.05, 1.0)


def parallel_frames(F, seed, lens=NEAR_PINHOLE):
    """A capture that cannot be calibrated: every frame parallel to the image plane, seen through a lens that is nearly a pinhole, so
    that nothing separates the focal length from the distance.  (Through a strongly distorting lens such a capture is not singular:
    the distortion itself fixes the scale, the homographies' capture-geometry test does not fire, and the solve goes ahead: DESIGN.md
    §4p has the measured ratios.)"""
    return M.make_case(lens, F, 0.05, seed, tilt_max=0.0)[0]


def test_frames_parallel_to_the_image_plane_have_no_start(K):
    p = K.params(NC.W, NC.H)
    for model in ("EUCM", "UCM"):
        for seed in range(3):
            win, outs = solve_all_starts(K, model, p, parallel_frames(4, seed))
            assert win == -1 and all(o[0]["status"] == A.CK_CALIB_DEGENERATE and o[0]["iters"] == 0 and not o[0]["cam"][:5].any() for o in outs)   # (UCM: slot 5 holds its 1.0)


def test_calibration_kernels_keep_their_budgets(built):
    """The code objects' own notes (llvm-readelf --notes, as test_fit_kernels_keep_their_register_budgets reads them): the EUCM
    calibration kernel uses no scratch and spills no vector register; the OpenCVModel5 kernel, whose code is to stay what it was, needs
    no more vector registers than before the kernel became a template: 390, read from a build of the commit before (which also had
    1832 bytes of LDS, no scratch and no vector spill; the EUCM kernel: 382 registers, the same LDS)."""
    from test_camera_host import _notes
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf in this image")
    build = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "chalkydri_amd", "csrc", "build")
    cv5 = [v for k, v in _notes(os.path.join(build, "k_calib.o")).items() if "k_calib" in k]
    eucm = [v for k, v in _notes(os.path.join(build, "k_calib_eucm.o")).items() if "k_calib" in k]
    assert len(cv5) == 1 and len(eucm) == 1, (cv5, eucm)
    print("OpenCVModel5", cv5[0], "EUCM", eucm[0])
    assert eucm[0]["private_segment_fixed_size"] == 0 and eucm[0]["vgpr_spill_count"] == 0
    assert cv5[0]["vgpr_count"] <= 390 and cv5[0]["private_segment_fixed_size"] == 0 and cv5[0]["vgpr_spill_count"] == 0
