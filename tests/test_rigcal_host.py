"""The host half of the mount calibration: ck_rigcal_refine_host (the bitwise specification of the device solver),
ck_rigcal_jacobian and ck_rigcal_check, against the truth and against tests/np_rigcal.py (numpy + scipy, Rodrigues rotations, numeric
Jacobians: no code shared with the library).  No GPU.

Inputs: room captures of 2 cameras x 40 steps and 3 cameras x 120 steps, seeds 0..4 of rigcal_cases.acceptance_case, bearing noise 0 and
1e-3: 20 cases.  Start mounts off by up to 5 degrees and 5 cm, start poses from ck_rig_solve_host with those mounts.  A distance between
two mounts is the larger of the angle between the rotations (rad) and the distance of the positions (m).  Bounds, each 100 times the
reference's own largest distance on these cases, measured once and fixed here:
  noise-free   scipy trf to the truth: 7.81e-16 at most -> BOUND_TRUTH = 7.9e-14 (the library: 1.92e-15 at most, STALLED at the floor of
               double precision after 35 .. 50 iterations; with §4j's cost threshold of 1e-20, which is px^2 there and rad^2 here, it
               stopped at 9.53e-11: see ck_rigcal_math.h, CKR_COST_FLOOR, which this bound pins)
  1e-3         scipy trf to scipy lm at the same minimum: 1.30e-9 at most -> BOUND_MINIMUM = 1.3e-7 (the library to trf: 1.29e-9 at most;
               its rms to trf's: 2.8e-18 at most, the issue's bound is 1e-9)
  Jacobian     central differences at step 1e-5 against step 5e-6, per column relative to the column's largest entry: 2.51e-10 at most
               -> BOUND_JACOBIAN = 2.6e-8 (the analytic Jacobian to the finer differences: 2.14e-10 at most)
All 20 cases end CONVERGED or STALLED (the noisy ones in at most 21 iterations)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_rigcal as N  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

BOUND_TRUTH, BOUND_MINIMUM, BOUND_JACOBIAN, BOUND_RMS = 7.9e-14, 1.3e-7, 2.6e-8, 1e-9
SHAPES = ((2, 40), (3, 120))
FIX0 = 0x3F


@pytest.fixture(scope="module")
def K(built):
    from chalkydri_amd import rigcal
    return rigcal


@functools.lru_cache(maxsize=None)
def _solved(n_cams, n_steps, seed, noise):
    """the case and the library's solve of it, once per session"""
    import rigcal_cases as RC
    from chalkydri_amd import rigcal as K
    cs = RC.acceptance_case(n_cams, n_steps, seed, noise)
    res, poses = K.refine_host(K.params(FIX0), K.Capture(cs["csteps"], [cs["ok"]]), cs["m0"], cs["poses0"])
    got = [RC.mount_of(K, res["robot_to_cam"][c]) for c in range(n_cams)]
    return cs, res, poses, got


def _dist(a, b):
    return max(max(N.mount_distance(x, y)) for x, y in zip(a, b))


def test_noise_free_recovery(K):
    """Every free mount against the truth on the 10 noise-free cases: scipy reaches it to 7.81e-16, the library to 1.92e-15."""
    worst = 0.0
    for n_cams, n_steps in SHAPES:
        for seed in range(5):
            cs, res, _, got = _solved(n_cams, n_steps, seed, 0.0)
            d = _dist(got, cs["mounts"])
            print(n_cams, n_steps, seed, "status", int(res["status"]), "iters", int(res["iters"]), "rms", float(res["rms"]), "to the truth", d)
            assert res["robot_to_cam"][0].tobytes() == bytes(cs["m0"][0])
            worst = max(worst, d)
    print("noise-free: the library to the truth", worst, "bound", BOUND_TRUTH)
    assert worst <= BOUND_TRUTH


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("seed", range(5))
def test_noisy_minimum_is_scipys(K, shape, seed):
    """bearing noise 1e-3: the mounts against scipy trf's minimum of the same cost from the same start, the rms against scipy's"""
    n_cams, n_steps = shape
    cs, res, poses, got = _solved(n_cams, n_steps, seed, 1e-3)
    ok = cs["ok"]
    prob = N.Problem([cs["steps"][s] for s in ok], n_cams)
    assert len(prob.used) == res["n_steps_used"] and len(prob.X) == res["n_points"]
    p0 = [(cs["poses0"][ok[u], :9].reshape(3, 3), cs["poses0"][ok[u], 9:]) for u in prob.used]
    sm, _, srms, _ = N.solve(prob, cs["start"], p0, [[False] * 6] + [[True] * 6] * (n_cams - 1))
    d = _dist(got, sm)
    print(shape, seed, "to scipy", d, "rms", float(res["rms"]), "scipy's", srms, "to the truth", _dist(got, cs["mounts"]), "start", _dist(cs["start"], cs["mounts"]))
    assert d <= BOUND_MINIMUM and abs(res["rms"] - srms) <= BOUND_RMS
    assert _dist(got, cs["mounts"]) < 0.1 * _dist(cs["start"], cs["mounts"])           # and that minimum is near the truth
    P = poses[prob.used]
    e = prob.residuals(np.stack([m[0] for m in got]), np.stack([m[1] for m in got]), P[:, :9].reshape(-1, 3, 3), P[:, 9:])
    cam = [np.sqrt(np.sum(e[prob.ci == c] ** 2) / np.sum(prob.ci == c)) for c in range(n_cams)]
    assert np.allclose(cam, res["cam_rms"][:n_cams], rtol=1e-6) and list(res["cam_points"][:n_cams]) == [int(np.sum(prob.ci == c)) for c in range(n_cams)]


def test_statuses(K):
    for noise in (0.0, 1e-3):
        for n_cams, n_steps in SHAPES:
            for seed in range(5):
                _, res, _, _ = _solved(n_cams, n_steps, seed, noise)
                assert res["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED), (noise, n_cams, n_steps, seed, int(res["status"]))
                assert res["cost"] <= res["cost0"] and np.isfinite(res["rms"]) and res["n_steps"] == len(_solved(n_cams, n_steps, seed, noise)[0]["ok"])


def test_analytic_jacobian(K):
    """40 random views of 8 points: ck_rigcal_jacobian against central differences, per column relative to its largest entry"""
    import rigcal_cases as RC
    rng = np.random.default_rng(1)
    worst = {"h": 0.0, "lib": 0.0}
    for _ in range(40):
        mounts = N.make_mounts(rng, 2)
        R, t = N.rot_z(rng.uniform(-3, 3)) @ N.small_rotation(rng, 0.2), rng.uniform(-3, 3, 3)
        Am, o = mounts[1]
        p = rng.uniform(-1, 1, (8, 3)) + np.array([0, 0, 3.0])
        X = ((p @ Am) + o - t) @ R                                           # world points in front of the camera
        v = p + rng.normal(0, 0.01, p.shape)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        pose = np.concatenate([R.reshape(9), t])
        r, J = K.jacobian(RC.mount_iso(mounts[1]), pose, X, v)
        J1, J2 = N.numeric_jacobian(mounts[1], (R, t), X, v, 1e-5), N.numeric_jacobian(mounts[1], (R, t), X, v, 5e-6)
        for k in range(12):
            big = np.abs(J2[:, :, k]).max()
            worst["h"] = max(worst["h"], np.abs(J1[:, :, k] - J2[:, :, k]).max() / big)
            worst["lib"] = max(worst["lib"], np.abs(J[:, :, k] - J2[:, :, k]).max() / big)
        pc = ((X @ R.T + t) - o) @ Am.T
        want = (pc - v * np.sum(v * pc, 1)[:, None]) / np.linalg.norm(pc, axis=1)[:, None]
        assert np.abs(r - want).max() < 1e-14
        _, Jf = K.jacobian(RC.mount_iso(mounts[1]), pose, X, v, fixed6=0b101001)
        assert not Jf[:, :, [0, 3, 5]].any() and np.array_equal(Jf[:, :, [1, 2, 4, 6, 7, 8, 9, 10, 11]], J[:, :, [1, 2, 4, 6, 7, 8, 9, 10, 11]])
    print("Jacobian: two step sizes", worst["h"], "analytic to the finer", worst["lib"])
    assert worst["lib"] <= BOUND_JACOBIAN


def test_frozen_dofs_and_the_gauge(K):
    """frozen dofs come back bit-unchanged; a camera with frozen position and free angles recovers its angles; a gauge-free mask is
    CK_EINVAL; a disconnected camera is DEGENERATE; steps with one camera are counted as skipped; a step without tags is harmless"""
    import rigcal_cases as RC
    cs, res_free, _, got_free = _solved(3, 120, 0, 0.0)
    steps, n = cs["csteps"], len(cs["csteps"])
    # camera 1: position frozen at the truth, angles off; camera 2 wholly frozen at the truth
    start = [cs["mounts"][0], (cs["start"][1][0], cs["mounts"][1][1]), cs["mounts"][2]]
    m0 = [RC.mount_iso(m) for m in start]
    p = K.params(FIX0 | K.fix_position(1) | K.fix_camera(2))
    res, _ = K.refine_host(p, K.Capture(steps, [cs["ok"]]), m0, cs["poses0"])
    assert res["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED)
    assert res["robot_to_cam"][0].tobytes() == bytes(m0[0]) and res["robot_to_cam"][2].tobytes() == bytes(m0[2])
    got1 = RC.mount_of(K, res["robot_to_cam"][1])
    assert np.abs(got1[1] - start[1][1]).max() < 1e-15                      # o comes back through b = -A o: round-off of the conversion
    ang0, ang1 = N.mount_distance(start[1], cs["mounts"][1])[0], N.mount_distance(got1, cs["mounts"][1])[0]
    print("frozen position: angle to the truth", ang0, "->", ang1)
    assert ang1 < 1e-6 * ang0
    # a rotation frozen: its quaternion comes back bit for bit while the position moves
    res, _ = K.refine_host(K.params(FIX0 | (0x07 << 6)), K.Capture(steps, [cs["ok"]]), cs["m0"], cs["poses0"])
    assert res["robot_to_cam"][1]["q"].tobytes() == bytes(cs["m0"][1])[24:] and res["robot_to_cam"][1]["t"].tobytes() != bytes(cs["m0"][1])[:24]
    # no gauge
    assert K.check(K.params(0), K.Capture(steps), cs["m0"]) == A.CK_EINVAL
    assert K.check(K.params(K.fix_position(0) | (K.fix_camera(1) & ~(1 << 6))), K.Capture(steps), cs["m0"]) == A.CK_EINVAL
    assert K.check(K.params(FIX0), K.Capture(steps), cs["m0"]) == A.CK_OK
    # a camera without a view in any used step stays as given and the others are solved
    empty = ([], np.zeros((0, 3)))
    two = [[cams[0], cams[1], empty] for cams in steps]
    res, poses = K.refine_host(K.params(FIX0), K.Capture(two, [cs["ok"]]), cs["m0"], cs["poses0"])
    assert res["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED) and res["cam_points"][2] == 0
    assert res["robot_to_cam"][2].tobytes() == bytes(cs["m0"][2])            # a camera without observations comes back as given
    # cameras 1 and 2 see each other's steps but never camera 0's: free cameras without a path to the fixed one
    island = [[cams[0], empty, empty] if s % 2 else [empty, cams[1], cams[2]] for s, cams in enumerate(steps)]
    res, poses = K.refine_host(K.params(FIX0), K.Capture(island, [cs["ok"]]), cs["m0"], cs["poses0"])
    assert res["status"] == A.CK_CALIB_DEGENERATE and res["iters"] == 0
    assert all(res["robot_to_cam"][c].tobytes() == bytes(cs["m0"][c]) for c in range(3)) and poses.tobytes() == cs["poses0"][cs["ok"]].tobytes()
    assert res["n_steps_used"] == sum(1 for s in cs["ok"] if not s % 2 and len(steps[s][1][0]) and len(steps[s][2][0]))
    # one-camera steps and a step without tags among the problem's steps: skipped and counted, their poses as given
    holes = [list(c) for c in steps]
    holes[cs["ok"][3]] = [empty, empty, empty]
    holes[cs["ok"][5]] = [steps[cs["ok"][5]][0], empty, empty]
    whole, _ = K.refine_host(K.params(FIX0), K.Capture(steps, [cs["ok"]]), cs["m0"], cs["poses0"])
    res, poses = K.refine_host(K.params(FIX0), K.Capture(holes, [cs["ok"]]), cs["m0"], cs["poses0"])
    lost = sum(1 for k in (3, 5) if sum(len(t) > 0 for t, _ in steps[cs["ok"][k]]) >= 2)
    assert res["status"] in (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED) and res["n_steps"] == whole["n_steps"]
    assert res["n_steps_used"] == whole["n_steps_used"] - lost
    assert poses[3].tobytes() == cs["poses0"][cs["ok"][3]].tobytes() and poses[5].tobytes() == cs["poses0"][cs["ok"][5]].tobytes()
    # fewer used steps than min_steps
    res, _ = K.refine_host(K.params(FIX0, min_steps=200), K.Capture(steps, [cs["ok"]]), cs["m0"], cs["poses0"])
    assert res["status"] == A.CK_CALIB_DEGENERATE


def test_refusals_in_their_order(K):
    """every refusal of ck_rigcal_check through Python; where two apply the earlier one of the documented order decides (the capacity,
    the last one, loses against a parameter out of range).  tests/cpp/rigcal_host_check.cpp walks the same list under the sanitizers."""
    import rigcal_cases as RC
    cs = RC.shape_case(1, 2, 5, lambda s, c: 1)
    steps, m0 = cs["csteps"], cs["m0"]
    ok = K.params(FIX0)
    assert K.check(ok, K.Capture(steps), m0) == A.CK_OK
    for bad in (K.params(FIX0, max_iters=0), K.params(FIX0, max_iters=10001), K.params(FIX0, min_steps=0), K.params(FIX0, min_cams_per_step=1),
                K.params(0), K.params(K.fix_position(0) | K.fix_position(1))):
        assert K.check(bad, K.Capture(steps), m0) == A.CK_EINVAL
    cap = K.Capture(steps, [[0, 2, 1]])
    assert K.check(ok, cap, m0) == A.CK_EINVAL                               # not increasing
    cap = K.Capture(steps, [[0, 1, 5]])
    assert K.check(ok, cap, m0) == A.CK_EINVAL                               # past the capture
    cap = K.Capture(steps)
    cap.records[1].n_bearings = 3
    assert K.check(ok, cap, m0) == A.CK_EINVAL                               # 4 n_tags != n_bearings
    cap = K.Capture(steps)
    cap.records[3].tag_offset = cap.n_tags
    assert K.check(ok, cap, m0) == A.CK_EINVAL                               # outside the arrays
    cap = K.Capture(steps)
    cap.bearings[4, 1] = np.nan
    assert K.check(ok, cap, m0) == A.CK_EINVAL
    nan_mount = [m0[0], A.Iso3.from_buffer_copy(m0[1])]
    nan_mount[1].t[0] = float("inf")
    assert K.check(ok, K.Capture(steps), nan_mount) == A.CK_EINVAL
    many = [steps[s % 5] for s in range(A.CK_RIGCAL_MAX_STEPS + 1)]
    assert K.check(ok, K.Capture(many), m0) == A.CK_ECAPACITY
    assert K.check(K.params(FIX0, max_iters=0), K.Capture(many), m0) == A.CK_EINVAL
    assert K.check(ok, K.Capture(many, [list(range(A.CK_RIGCAL_MAX_STEPS))]), m0) == A.CK_OK
