"""The host half of the field calibration: ck_fieldcal_refine_host (the bitwise specification of the device solver),
ck_fieldcal_jacobian and ck_fieldcal_check, against the truth and against tests/np_fieldcal.py (numpy + scipy, Rodrigues rotations,
numeric Jacobians: no code shared with the library).  No GPU.

Inputs: room captures (8 x 6 m, 28 wall tags) of 1 camera x 60 steps, 2 cameras x 40 steps and 3 cameras x 40 steps, seeds 0 and 1
of fieldcal_cases.acceptance_case, bearing noise 0 and 1e-3: 12 cases.  The true layout is the nominal one with every tag but the
gauge moved by up to 3 cm and 2 degrees; the starts are the nominal layout and the poses of ck_rig_solve_host with it.  A distance
between two layouts is the largest, over the tags with sightings, of the angle between the rotations (rad) and the distance of the
positions (m).  Bounds, each 100 times the reference's own largest distance on these cases, measured once and fixed here:
  noise-free   scipy trf to the truth: 1.51e-14 at most -> BOUND_TRUTH = 1.51e-12 (the library: 6.00e-14 at most, in 46 .. 55 iterations, STALLED at the
               floor of double precision; CKR_COST_FLOOR of §4l is what lets it get there)
  1e-3         scipy trf to scipy lm at the same minimum: 5.18e-8 at most -> BOUND_MINIMUM = 5.2e-6 (the library to trf:
               1.31e-7 at most, in 11 .. 27 iterations; its rms to trf's, relative: 2.9e-15 at most, the issue's bound is 1e-9)
  Jacobian     central differences at step 1e-5 against step 5e-6, per column relative to the column's largest entry:
               7.99e-9 at most -> BOUND_JACOBIAN = 8.0e-7 (the analytic Jacobian to the finer differences: 7.63e-9 at most)
All 12 cases end CONVERGED or STALLED."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_fieldcal as N  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

BOUND_TRUTH, BOUND_MINIMUM, BOUND_JACOBIAN, BOUND_RMS = 1.51e-12, 5.2e-6, 8.0e-7, 1e-9
SHAPES = ((1, 60), (2, 40), (3, 40))
SEEDS = (0, 1)
DONE = (A.CK_CALIB_CONVERGED, A.CK_CALIB_STALLED)


@pytest.fixture(scope="module")
def K(built):
    from chalkydri_amd import fieldcal
    return fieldcal


@functools.lru_cache(maxsize=None)
def _solved(n_cams, n_steps, seed, noise):
    """the case and the library's solve of it, once per session"""
    import fieldcal_cases as FC
    from chalkydri_amd import fieldcal as K
    cs = FC.acceptance_case(n_cams, n_steps, seed, noise)
    res, lay, sight, rms, poses = K.refine_host(K.params(), K.Capture(cs["steps"], [cs["ok"]]), cs["m_iso"], cs["lay0"], cs["fixed"], cs["poses0"])
    return cs, res, lay, sight, rms, poses, FC.layout_of(lay)


@functools.lru_cache(maxsize=None)
def _scipy(n_cams, n_steps, seed, noise, method):
    """scipy's minimum of the same case from the same start"""
    cs = _solved(n_cams, n_steps, seed, noise)[0]
    ok = cs["ok"]
    prob = N.Problem([cs["steps"][s] for s in ok], cs["mounts"], len(cs["nominal"]))
    p0 = [(cs["poses0"][ok[u], :9].reshape(3, 3), cs["poses0"][ok[u], 9:]) for u in prob.used]
    free = [[bool(prob.sightings[k] > 0 and k != cs["gauge"])] * 6 for k in range(len(cs["nominal"]))]
    lay, poses, rms, _ = N.solve(prob, cs["nominal"], p0, free, method=method)
    return prob, lay, poses, rms


def test_noise_free_recovery(K):
    """Every tag with sightings against the truth on the 6 noise-free cases, the library and scipy trf"""
    worst, ref = 0.0, 0.0
    for n_cams, n_steps in SHAPES:
        for seed in SEEDS:
            cs, res, lay, sight, _, _, got = _solved(n_cams, n_steps, seed, 0.0)
            seen = [k for k in range(len(got)) if sight[k] > 0]
            _, sl, _, _ = _scipy(n_cams, n_steps, seed, 0.0, "trf")
            d, ds = N.layout_distance(got, cs["true"], seen), N.layout_distance(sl, cs["true"], seen)
            print(n_cams, n_steps, seed, "status", int(res["status"]), "iters", int(res["iters"]), "rms", float(res["rms"]), "to the truth", d, "scipy trf", ds)
            assert res["status"] in DONE and lay[cs["gauge"]].tobytes() == bytes(cs["lay0"][cs["gauge"]])
            worst, ref = max(worst, d), max(ref, ds)
    print("noise-free: the library to the truth", worst, "scipy trf", ref, "bound", BOUND_TRUTH)
    assert worst <= BOUND_TRUTH


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_noisy_minimum_is_scipys(K, shape, seed):
    """bearing noise 1e-3: the layout against scipy trf's minimum of the same cost from the same start, the rms against scipy's, the
    per-tag records against numpy's"""
    n_cams, n_steps = shape
    cs, res, lay, sight, rms, poses, got = _solved(n_cams, n_steps, seed, 1e-3)
    prob, sl, _, srms = _scipy(n_cams, n_steps, seed, 1e-3, "trf")
    _, ll, _, _ = _scipy(n_cams, n_steps, seed, 1e-3, "lm")
    seen = [k for k in range(len(got)) if sight[k] > 0]
    assert res["status"] in DONE and len(prob.used) == res["n_steps_used"] and len(prob.x) == res["n_points"]
    assert list(sight) == list(prob.sightings) and res["n_tags_solved"] == len(seen) - 1
    d = N.layout_distance(got, sl, seen)
    print(shape, seed, "to scipy trf", d, "trf to lm", N.layout_distance(sl, ll, seen), "rms", float(res["rms"]), "scipy's", srms, "relative",
          abs(res["rms"] - srms) / srms, "iters", int(res["iters"]))
    assert d <= BOUND_MINIMUM and abs(res["rms"] - srms) <= BOUND_RMS * srms
    P = poses[prob.used]
    want = prob.tag_rms(np.stack([m[0] for m in got]), np.stack([m[1] for m in got]), P[:, :9].reshape(-1, 3, 3), P[:, 9:])
    assert np.allclose(rms, want, rtol=1e-6, atol=0) and res["cost"] <= res["cost0"]


def test_analytic_jacobian(K):
    """40 random sightings: ck_fieldcal_jacobian against central differences, per column relative to its largest entry"""
    import fieldcal_cases as FC
    rng = np.random.default_rng(1)
    worst = {"h": 0.0, "lib": 0.0}
    keep = [1, 2, 4, 6, 7, 8, 9, 10, 11]
    for _ in range(40):
        mount = N.make_mounts(rng, 2)[1]
        Am, o = mount
        R, t = N.rot_z(rng.uniform(-3, 3)) @ N.small_rotation(rng, 0.2), rng.uniform(-3, 3, 3)
        pc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 5)])           # the tag in front of the camera
        Q, c = N.random_rotation(rng), ((pc @ Am) + o - t) @ R
        p = (((N.CORNERS @ Q.T + c) @ R.T + t) - o) @ Am.T
        v = p + rng.normal(0, 0.01, p.shape)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        pose = np.concatenate([R.reshape(9), t])
        r, J = K.jacobian(FC.mount_iso(mount), pose, FC.iso(Q, c), v)
        J1, J2 = N.numeric_jacobian(mount, (R, t), (Q, c), v, 1e-5), N.numeric_jacobian(mount, (R, t), (Q, c), v, 5e-6)
        for k in range(12):
            big = np.abs(J2[:, :, k]).max()
            worst["h"] = max(worst["h"], np.abs(J1[:, :, k] - J2[:, :, k]).max() / big)
            worst["lib"] = max(worst["lib"], np.abs(J[:, :, k] - J2[:, :, k]).max() / big)
        want = (p - v * np.sum(v * p, 1)[:, None]) / np.linalg.norm(p, axis=1)[:, None]
        assert np.abs(r - want).max() < 1e-14
        _, Jf = K.jacobian(FC.mount_iso(mount), pose, FC.iso(Q, c), v, fixed6=0b101001)
        assert not Jf[:, :, [0, 3, 5]].any() and np.array_equal(Jf[:, :, keep], J[:, :, keep])
        r3, J3 = K.jacobian(FC.mount_iso(mount), pose, FC.iso(Q, c), v[:3])
        assert np.array_equal(r3, r[:3]) and np.array_equal(J3, J[:3])
    print("Jacobian: two step sizes", worst["h"], "analytic to the finer", worst["lib"], "bound", BOUND_JACOBIAN)
    assert worst["lib"] <= BOUND_JACOBIAN


def test_frozen_parts_the_gauge_and_degenerate_problems(K):
    """frozen parts come back bit for bit (a whole tag, a quaternion only, single position axes); an unseen tag is returned as given;
    no wholly frozen tag with sightings is CK_EINVAL; a free tag without a chain of shared steps to a frozen one is DEGENERATE;
    one-tag steps are skipped and counted"""
    import fieldcal_cases as FC
    cs = _solved(3, 40, 0, 1e-3)[0]
    steps, ok, L, g = cs["steps"], cs["ok"], len(cs["nominal"]), cs["gauge"]
    sight0 = _solved(3, 40, 0, 1e-3)[3]
    a, b, c = [k for k in np.argsort(-sight0) if k != g][:3]
    fx = cs["fixed"].copy()
    fx[a], fx[b], fx[c] = 63, K.FIX_ROTATION, 0b010000 | 0b100000                 # whole; quaternion; y and z of the position
    res, lay, sight, rms, _ = K.refine_host(K.params(), K.Capture(steps, [ok]), cs["m_iso"], cs["lay0"], fx, cs["poses0"])
    assert res["status"] in DONE and res["n_tags_solved"] == np.sum(sight > 0) - 2
    raw = lambda iso: np.frombuffer(bytes(iso), np.float64)
    assert lay[a].tobytes() == bytes(cs["lay0"][a]) and lay[g].tobytes() == bytes(cs["lay0"][g])
    assert lay[b]["q"].tobytes() == raw(cs["lay0"][b])[3:].tobytes() and not np.array_equal(lay[b]["t"], raw(cs["lay0"][b])[:3])
    assert np.array_equal(lay[c]["t"][1:], raw(cs["lay0"][c])[1:3]) and lay[c]["t"][0] != raw(cs["lay0"][c])[0]
    assert not np.array_equal(lay[c]["q"], raw(cs["lay0"][c])[3:])
    # a layout entry without a sighting: as given, sightings 0, rms 0
    more = cs["lay0"] + [FC.iso(np.eye(3), [1.0, 2.0, 3.0])]
    res, lay, sight, rms, _ = K.refine_host(K.params(), K.Capture(steps, [ok]), cs["m_iso"], more, np.append(cs["fixed"], 0), cs["poses0"])
    assert res["status"] in DONE and lay[L].tobytes() == bytes(more[L]) and sight[L] == 0 and rms[L] == 0
    assert lay[:L].tobytes() == _solved(3, 40, 0, 1e-3)[2].tobytes()
    # the gauge
    assert K.check(K.params(), K.Capture(steps), cs["m_iso"], cs["lay0"], np.zeros(L, np.uint8)) == A.CK_EINVAL
    assert K.check(K.params(), K.Capture(steps), cs["m_iso"], cs["lay0"], FC.fixed_of(L, {g: 0b111110})) == A.CK_EINVAL
    assert K.check(K.params(), K.Capture(steps), cs["m_iso"], more, FC.fixed_of(L + 1, {L: 63})) == A.CK_EINVAL   # frozen, never seen
    assert K.check(K.params(), K.Capture(steps), cs["m_iso"], cs["lay0"], cs["fixed"]) == A.CK_OK
    # an island: the steps keep either tags below 14 or tags from 14 on, so the half without the gauge hangs on nothing
    half = lambda ids, bear, lo: ([k for k in ids if (k < 14) == lo], np.concatenate([bear[4 * j:4 * j + 4] for j, k in enumerate(ids) if (k < 14) == lo] + [np.zeros((0, 3))]))
    island = [[half(ids, bear, bool(s % 2)) for ids, bear in cams] for s, cams in enumerate(steps)]
    res, lay, sight, rms, poses = K.refine_host(K.params(), K.Capture(island, [ok]), cs["m_iso"], cs["lay0"], cs["fixed"], cs["poses0"])
    assert res["status"] == A.CK_CALIB_DEGENERATE and res["iters"] == 0 and res["n_steps_used"] > 3
    assert lay.tobytes() == b"".join(bytes(t) for t in cs["lay0"]) and poses.tobytes() == cs["poses0"][ok].tobytes() and not rms.any()
    # one-tag steps and a step without tags among the problem's steps: skipped and counted, their poses as given
    empty = ([], np.zeros((0, 3)))
    holes = [list(cams) for cams in steps]
    holes[ok[3]] = [empty] * 3
    first = next(cam for cam in steps[ok[5]] if len(cam[0]))
    holes[ok[5]] = [([first[0][0]], first[1][:4]), ([first[0][0]], first[1][:4]), empty]                     # one tag, seen by two cameras
    whole = _solved(3, 40, 0, 1e-3)[1]
    res, _, _, _, poses = K.refine_host(K.params(), K.Capture(holes, [ok]), cs["m_iso"], cs["lay0"], cs["fixed"], cs["poses0"])
    lost = sum(1 for k in (3, 5) if len({t for ids, _ in steps[ok[k]] for t in ids}) >= 2)
    assert res["status"] in DONE and res["n_steps"] == whole["n_steps"] and res["n_steps_used"] == whole["n_steps_used"] - lost
    assert poses[3].tobytes() == cs["poses0"][ok[3]].tobytes() and poses[5].tobytes() == cs["poses0"][ok[5]].tobytes()
    # fewer used steps than min_steps; a start that is not finite
    res = K.refine_host(K.params(min_steps=200), K.Capture(steps, [ok]), cs["m_iso"], cs["lay0"], cs["fixed"], cs["poses0"])[0]
    assert res["status"] == A.CK_CALIB_DEGENERATE
    bad = cs["poses0"].copy()
    bad[next(s for s in ok if len({t for ids, _ in steps[s] for t in ids}) >= 2), 4] = np.nan
    res = K.refine_host(K.params(), K.Capture(steps, [ok]), cs["m_iso"], cs["lay0"], cs["fixed"], bad)[0]
    assert res["status"] == A.CK_CALIB_DEGENERATE


def test_one_camera(K):
    """a robot with a single camera: the layout comes back nearer the truth than the drawing, noise-free to round-off"""
    cs, res, _, sight, _, _, got = _solved(1, 60, 0, 0.0)
    seen = [k for k in range(len(got)) if sight[k] > 0]
    assert cs["n_cams"] == 1 and res["status"] in DONE and len(seen) > 10
    assert N.layout_distance(got, cs["true"], seen) < 1e-9 < 1e-3 < N.layout_distance(cs["nominal"], cs["true"], seen)


def test_refusals_in_their_order(K):
    """every refusal of ck_fieldcal_check through Python; where two apply the earlier one of the documented order decides.
    tests/cpp/fieldcal_host_check.cpp walks the same list under the sanitizers."""
    import fieldcal_cases as FC
    cs = FC.shape_case(1, 2, 5, 4, FC.ring(4, 2))
    steps, m, lay, fx = cs["steps"], cs["m_iso"], cs["lay0"], cs["fixed"]
    ok = K.params()
    chk = lambda p=ok, cap=None, mounts=m, layout=lay, fixed=fx: K.check(p, K.Capture(steps) if cap is None else cap, mounts, layout, fixed)
    assert chk() == A.CK_OK
    cap = K.Capture(steps)
    cap.records[3].tag_offset = cap.n_tags
    assert chk(cap=cap) == A.CK_EINVAL                                       # (3) outside the arrays
    cap = K.Capture(steps)
    cap.records[1].n_bearings = 3
    assert chk(cap=cap) == A.CK_EINVAL                                       # (4) 4 n_tags != n_bearings
    cap = K.Capture(steps)
    cap.tag_index[2] = 4
    assert chk(cap=cap) == A.CK_EINVAL                                       # (5) not an entry of the layout
    assert chk(cap=K.Capture(steps, [[0, 2, 1]])) == A.CK_EINVAL             # (6) not increasing
    assert chk(cap=K.Capture(steps, [[0, 1, 5]])) == A.CK_EINVAL             #     past the capture
    for bad in (K.params(max_iters=0), K.params(max_iters=10001), K.params(min_steps=0), K.params(min_tags_per_step=1)):
        assert chk(p=bad) == A.CK_EINVAL                                     # (7)
    assert chk(fixed=FC.fixed_of(4, {0: 63, 1: 64})) == A.CK_EINVAL
    cap = K.Capture(steps)
    cap.bearings[4, 1] = np.nan
    assert chk(cap=cap) == A.CK_EINVAL                                       # (8)
    nan_mount = [m[0], A.Iso3.from_buffer_copy(m[1])]
    nan_mount[1].t[0] = float("inf")
    assert chk(mounts=nan_mount) == A.CK_EINVAL
    nan_lay = list(lay[:3]) + [A.Iso3.from_buffer_copy(lay[3])]
    nan_lay[3].q[2] = float("nan")
    assert chk(layout=nan_lay) == A.CK_EINVAL
    cap = K.Capture(steps)
    cap.tag_index[1] = cap.tag_index[0]
    assert chk(cap=cap) == A.CK_EINVAL                                       # (9) the same tag twice in one view
    assert chk(fixed=np.zeros(4, np.uint8)) == A.CK_EINVAL                   # (10) no gauge
    many = [steps[s % 5] for s in range(A.CK_FIELDCAL_MAX_STEPS + 1)]
    assert chk(cap=K.Capture(many)) == A.CK_ECAPACITY                        # (11)
    assert chk(p=K.params(max_iters=0), cap=K.Capture(many)) == A.CK_EINVAL  # the earlier one decides
    assert chk(fixed=np.zeros(4, np.uint8), cap=K.Capture(many)) == A.CK_EINVAL
    assert chk(cap=K.Capture(many, [list(range(A.CK_FIELDCAL_MAX_STEPS))])) == A.CK_OK
    wide = FC.shape_case(2, 1, 2, 65, lambda s, c: range(65) if s == 0 else range(64))
    assert K.check(ok, K.Capture(wide["steps"]), wide["m_iso"], wide["lay0"], wide["fixed"]) == A.CK_ECAPACITY       # 65 tags in one problem
    assert K.check(ok, K.Capture(wide["steps"], [[1]]), wide["m_iso"], wide["lay0"], wide["fixed"]) == A.CK_OK
