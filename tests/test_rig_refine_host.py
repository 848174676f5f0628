"""The rig pose refinement on the host (ck_rig_refine_host, chalkydri_amd/csrc/ck_rig_refine_host.c) against its numpy
restatement (tests/np_rig_refine.py): the minimum against scipy's, the covariance against finite differences, its consistency and the
accuracy against today's fused pose by Monte Carlo, the rejection masks, the frozen behaviour, the refusals, the code object of the
kernel that runs the same arithmetic and the twin under sanitizers.  No device is needed: the kernel is compared with this twin in
tests/test_gpu_rig_refine.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_rig as N  # noqa: E402
import np_rig_refine as F  # noqa: E402
import np_rig_robust as NR  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd.rig import REFINED_DTYPE, RESULT_DTYPE, RefineParams, RigSolver, pack_steps  # noqa: E402
from chalkydri_amd.sqpnp import iso3  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN = os.path.join(ROOT, "chalkydri_amd", "lib", "rig_refine_asan")
DRAWS = 2000
GYRO_SIGMA = 0.01
WELL_POSED = ("near_far", "wall", "two_cameras")


def to_step(cams):
    return [([iso3(t, N.mat_to_quat(R)) for R, t in tags], b, iso3(bb, N.mat_to_quat(Am))) for tags, b, (Am, bb) in cams]


def start_record(R_wr, p):
    st = np.zeros(1, RESULT_DTYPE)
    st["valid"], st["rot"], st["pos"] = 1, R_wr, p
    return st


def yaw_of(rot):
    return np.arctan2(rot[..., 1, 0], rot[..., 0, 0])


@pytest.fixture(scope="module")
def solver(built):
    return RigSolver()


@pytest.fixture(scope="module")
def noisy(solver):
    """one noisy draw of every well-posed scene with its fused start, shared by the minimum and the covariance tests"""
    rng = np.random.default_rng(11)
    out = {}
    for name in WELL_POSED:
        cams = F.render(F.SCENES[name], rng, F.NOISE)
        gyro = F.TRUTH[2] + rng.normal(0, GYRO_SIGMA)
        st = solver.solve_host([to_step(cams)], [gyro])
        assert st["valid"][0]
        out[name] = (cams, gyro, st)
    return out


CONFIGS = [(mode, gs) for mode in (F.FREE, F.PLANAR) for gs in (0.0, GYRO_SIGMA)]


def test_minimum_matches_scipy(solver, noisy):
    """The twin's pose is scipy's minimum of the restated cost from the same start, to 1e-9 (m, rad), in both modes, with and without
    the prior.  The scenes are the well-posed ones: a single far tag leaves a valley along which double precision does not determine the
    minimum to 1e-9 (the twin and scipy differ by up to 3e-7 there)."""
    for name, (cams, gyro, st) in noisy.items():
        for mode, gs in CONFIGS:
            r = solver.refine_host([to_step(cams)], [gyro], st, RefineParams(planar=mode == F.PLANAR, sigma=F.NOISE, gyro_sigma=gs, max_iters=50))[0]
            R, p, cost = F.minimise(cams, st[0]["rot"], st[0]["pos"], mode, F.NOISE, gyro, gs, 0.0)
            d = (np.abs(r["rot"] - R).max(), np.abs(r["pos"] - p).max(), abs(yaw_of(r["rot"]) - yaw_of(R)))
            print(name, mode, gs, "iters", r["iters"], "d rot %.1e pos %.1e yaw %.1e" % d)
            assert r["status"] == A.CK_RIG_REFINE_CONVERGED and max(d) < 1e-9, (name, mode, gs, d)
            assert abs(r["cost"] - cost) <= 1e-9 * cost and (gs > 0 or r["cost0"] >= r["cost"])
            assert r["n_points"] == 4 * sum(len(c[0]) for c in cams) and r["dof"] == 2 * r["n_points"] + (gs > 0) - (3 if mode else 6)
            assert abs(r["rms"] - np.sqrt(r["cost"] / r["n_points"])) < 1e-15


def test_noise_free_returns_the_truth(solver):
    """exact bearings, a start 2 cm and 0.6 degrees off: the truth to 1e-12, CONVERGED"""
    R_t, p_t = F.truth_pose()
    for name in WELL_POSED + ("single_3m",):
        cams = F.render(F.SCENES[name])
        st = start_record(F.exp_so3(np.array([0.004, -0.003, 0.01])) @ R_t, p_t + np.array([0.02, -0.015, 0.01]))
        for mode, gs in CONFIGS:
            if name == "single_3m" and mode == F.FREE:
                continue                             # (one tag, six unknowns: the planar ambiguity's valley, see test_minimum_matches_scipy)
            r = solver.refine_host([to_step(cams)], [F.TRUTH[2]], st, RefineParams(planar=mode == F.PLANAR, gyro_sigma=gs, max_iters=100))[0]
            d = (np.abs(r["rot"] - R_t).max(), np.abs(r["pos"] - p_t).max())
            print(name, mode, gs, "iters", r["iters"], "d rot %.1e pos %.1e" % d, "cost %.1e" % r["cost"])
            assert r["status"] == A.CK_RIG_REFINE_CONVERGED and max(d) < 1e-12, (name, mode, gs, d)
            assert r["moved_m"] > 0.01 and abs(r["moved_rad"] - 2 * np.sin(np.arccos((np.trace(st[0]["rot"].T @ r["rot"]) - 1) / 2) / 2)) < 1e-9


def test_covariance_is_the_inverse_normal_matrix(solver, noisy):
    """cov = sigma^2 (J^T J)^-1 with J by central differences in the world-axes tangent (the prior's row included), 1e-6 relative on
    every entry that is not zero (|C_ij| > 1e-9 sqrt(C_ii C_jj)); in planar mode the rows and columns of z, wx, wy are exactly zero"""
    for name, (cams, gyro, st) in noisy.items():
        for mode, gs in CONFIGS:
            r = solver.refine_host([to_step(cams)], [gyro], st, RefineParams(planar=mode == F.PLANAR, sigma=F.NOISE, gyro_sigma=gs, max_iters=50))[0]
            Cref = F.covariance(cams, r["rot"], r["pos"], mode, F.NOISE, gyro, gs)
            keep = [0, 1, 5] if mode == F.PLANAR else list(range(6))
            dg = np.sqrt(np.diag(Cref))
            worst = 0.0
            for i in keep:
                for j in keep:
                    if abs(Cref[i, j]) > 1e-9 * dg[i] * dg[j]:
                        worst = max(worst, abs(r["cov"][i, j] - Cref[i, j]) / abs(Cref[i, j]))
            print(name, mode, gs, "worst relative %.1e" % worst)
            assert worst < 1e-6 and np.array_equal(r["cov"], r["cov"].T)
            if mode == F.PLANAR:
                fixed = [2, 3, 4]
                assert not r["cov"][fixed, :].any() and not r["cov"][:, fixed].any()
            assert np.array_equal(r["std_devs"], np.sqrt(np.diag(r["cov"])[[0, 1, 5]]))


# ---- Monte Carlo ---------------------------------------------------------------------------------------------------------------------
def draws(name, seed, n=DRAWS):
    """n noisy instants of a scene (bearing noise 5e-4 per component, heading noise GYRO_SIGMA) as RigSolver takes them"""
    rng = np.random.default_rng(seed)
    isos = [([iso3(t, N.mat_to_quat(np.asarray(R, float))) for R, t in tags], iso3(b, N.mat_to_quat(Am))) for (Am, b), tags in F.SCENES[name]]
    steps, gyro = [], []
    for _ in range(n):
        cams = F.render(F.SCENES[name], rng, F.NOISE)
        steps.append([(isos[c][0], cams[c][1], isos[c][1]) for c in range(len(cams))])
        gyro.append(F.TRUTH[2] + rng.normal(0, GYRO_SIGMA))
    return steps, np.array(gyro)


@pytest.fixture(scope="module")
def monte_carlo(solver):
    """every scene's draws through ck_rig_solve_host once, and the refinements the tests ask for, each once"""
    cache = {}

    def get(name, planar=None, gs=0.0):
        if name not in cache:
            steps, gyro = draws(name, 7)
            st = solver.solve_host(steps, gyro)
            assert st["valid"].all()
            cache[name] = (steps, gyro, st)
        steps, gyro, st = cache[name]
        if planar is None:
            return st
        key = (name, planar, gs)
        if key not in cache:
            cache[key] = solver.refine_host(steps, gyro, st, RefineParams(planar=planar, sigma=F.NOISE, gyro_sigma=gs, max_iters=30))
        return cache[key]
    return get


def errors(rec):
    return rec["pos"][:, 0] - F.TRUTH[0], rec["pos"][:, 1] - F.TRUTH[1], yaw_of(rec["rot"]) - F.TRUTH[2]


# (scene, planar, gyro sigma).  The single far tag without a prior is left out on purpose: its linearisation fails (predicted over
# empirical 1.33 / 1.20 / 1.20 in planar mode, 1.41 / 0.73 / 0.73 with six unknowns, measured with this twin), which is what the
# prior is for; so is the single 3 m tag without one (1.22 / 0.99 / 0.99 planar).  Every scene listed was measured within the bound
# on the twin before the list was fixed: ratios between 0.971 and 1.024, mean chi2 between 0.983 and 1.000 (the wall with six unknowns
# and no prior, the issue's "three-tag wall" as it stands: 0.997 / 1.023 / 1.020, chi2 0.996).
CONSISTENT = [("near_far", False, 0.0), ("near_far", True, 0.0), ("wall", False, 0.0), ("wall", True, 0.0), ("wall", False, GYRO_SIGMA), ("two_cameras", False, 0.0),
              ("two_cameras", True, GYRO_SIGMA), ("single_3m", True, GYRO_SIGMA), ("far_single", True, GYRO_SIGMA)]


@pytest.mark.parametrize("name,planar,gs", CONSISTENT)
def test_covariance_is_consistent(monte_carlo, name, planar, gs):
    """Over 2000 draws every predicted standard deviation (x, y, yaw; the root mean square of std_devs) lies within 10 % of the empirical
    one (the sampling error of a standard deviation at N = 2000 is 1.6 %: six of those) and the mean chi2 within 5 % of 1."""
    r = monte_carlo(name, planar, gs)
    assert (r["status"] <= A.CK_RIG_REFINE_MAXITERS).all()
    emp = np.array([e.std() for e in errors(r)])
    pred = np.sqrt(np.mean(r["std_devs"] ** 2, axis=0))
    print(name, planar, gs, "predicted", pred, "empirical", emp, "ratio", pred / emp, "chi2", r["chi2"].mean())
    assert np.abs(pred / emp - 1).max() < 0.10
    assert abs(r["chi2"].mean() - 1) < 0.05


def test_max_iters_is_not_a_quality_gate(monte_carlo, solver):
    """The coplanar wall with six unknowns is the scene on which the default max_iters ends most draws MAXITERS (1412 of 2000 when this
    was written): the damping is still coming down when the count runs out.  The header promises that such a record is as usable as a
    CONVERGED one.  Usable is measured against what a consumer weighs the pose by, its own standard deviations: against the
    30-iteration run of the same draws no component of the position and no yaw is off by more than a thousandth of its predicted
    standard deviation (a change no estimator that weighs by those sigmas can see in three digits), and no standard deviation by more
    than a thousandth of itself.  Measured when written: 4.8e-6 sigma at worst (2.0e-7 m), yaw 2.3e-6 sigma, std_devs 1.6e-7 relative."""
    long = monte_carlo("wall", False, 0.0)
    steps, gyro = draws("wall", 7)
    short = solver.refine_host(steps, gyro, monte_carlo("wall"), RefineParams(sigma=F.NOISE))
    n_max = int((short["status"] == A.CK_RIG_REFINE_MAXITERS).sum())
    sig = np.sqrt(np.stack([long["cov"][:, i, i] for i in range(3)], axis=1))
    dp = (np.abs(short["pos"] - long["pos"]) / sig).max()
    dw = (np.abs(yaw_of(short["rot"]) - yaw_of(long["rot"])) / long["std_devs"][:, 2]).max()
    ds = np.abs(short["std_devs"] / long["std_devs"] - 1).max()
    print("MAXITERS at the default 10:", n_max, "of", len(short), "; against 30 iterations: position %.1e sigma (%.1e m), yaw %.1e sigma, std_devs relative %.1e"
          % (dp, np.abs(short["pos"] - long["pos"]).max(), dw, ds))
    assert (short["status"] <= A.CK_RIG_REFINE_MAXITERS).all() and n_max > 0 and (short["iters"] <= 10).all()
    assert dp < 1e-3 and dw < 1e-3 and ds < 1e-3


def test_twin_is_reentrant(monte_carlo, solver):
    """ck_rig_refine_host keeps no state between or across calls: four threads refining the same 2000 draws at once (ctypes releases the
    interpreter lock for the call), in different modes, each return the bytes of the same call made alone."""
    import threading
    steps, gyro = draws("near_far", 7)
    start = monte_carlo("near_far")
    n_cams, probs, tarr, nt, barr = pack_steps(steps)
    L = solver._L
    prms = [RefineParams(planar=p, sigma=F.NOISE, gyro_sigma=g, max_iters=30)._c(L) for p, g in ((False, 0.0), (True, 0.0), (False, GYRO_SIGMA), (True, GYRO_SIGMA))]

    def run(prm, out):
        rc = L.ck_rig_refine_host(C.byref(prm), n_cams, probs, len(steps), tarr, nt, barr.ctypes.data, len(barr), gyro.ctypes.data, start.ctypes.data,
                                  None, out.ctypes.data_as(C.POINTER(A.RigRefined)))
        assert rc == A.CK_OK
    alone = [np.zeros(len(steps), REFINED_DTYPE) for _ in prms]
    for prm, out in zip(prms, alone):
        run(prm, out)
    assert alone[0].tobytes() == monte_carlo("near_far", False, 0.0).tobytes()
    differ = 0
    for _ in range(5):
        together = [np.zeros(len(steps), REFINED_DTYPE) for _ in prms]
        threads = [threading.Thread(target=run, args=(prm, out)) for prm, out in zip(prms, together)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        differ += sum(a.tobytes() != b.tobytes() for a, b in zip(alone, together))
    assert differ == 0


def rms_errors(rec):
    ex, ey, ew = errors(rec)
    return np.sqrt(np.mean(ex * ex) + np.mean(ey * ey)), np.sqrt(np.mean(ew * ew))


# The gains the twin showed on these draws (RMS xy in metres, RMS yaw in radians), from which the bounds below are taken:
#               fused            free             planar           planar + prior 0.01
#   near_far    0.0083 0.00079   0.0056 0.00056   0.0021 0.00036   -
#   wall        0.0114 0.00209   0.0114 0.00209   0.0060 0.00176   -
#   far_single  0.6954 0.10535   1.0340 0.16680   0.7740 0.12917   0.0622 0.00994
# (better, worse, scene, gain in xy, gain in yaw); a gain the twin showed below 10 % is None: reported, not asserted.
FUSED, FREE6, PLANAR3, PRIOR = "fused", (False, 0.0), (True, 0.0), (True, GYRO_SIGMA)
COMPARISONS = [(FREE6, FUSED, "near_far", 0.0027, 0.00023), (PLANAR3, FREE6, "near_far", 0.0035, 0.00020), (PLANAR3, FREE6, "wall", 0.0054, 0.00033),
               (PLANAR3, FREE6, "far_single", 0.2600, 0.03763), (PRIOR, PLANAR3, "far_single", 0.7118, 0.11923), (FREE6, FUSED, "wall", None, None)]


@pytest.mark.parametrize("better,worse,name,gain_xy,gain_yaw", COMPARISONS)
def test_accuracy_against_todays_pose(monte_carlo, better, worse, name, gain_xy, gain_yaw):
    """The same draws through ck_rig_solve_host, then the refinement: the better configuration's RMS error lies below the other's, as
    measured here, by at least half the gain the twin showed when the table above was written.  `fused` is ck_rig_solve_host's pose."""
    def get(which):
        return rms_errors(monte_carlo(name) if which == FUSED else monte_carlo(name, *which))
    b, w = get(better), get(worse)
    print(name, "fused xy %.4f yaw %.5f;" % get(FUSED), worse, "xy %.4f yaw %.5f;" % w, better, "xy %.4f yaw %.5f" % b)
    if gain_xy is not None:
        assert b[0] <= w[0] - 0.5 * gain_xy and b[1] <= w[1] - 0.5 * gain_yaw


# ---- masks, frozen behaviour, misuse ---------------------------------------------------------------------------------------------------
def test_rejected_tags_are_deleted_tags(solver):
    """refining a robust record with rejected tags returns the bytes of refining the same input with those tags deleted"""
    n = 0
    for k, v in NR.suite().items():
        planted = [c for c in v if any(c["planted"])][:3]
        if not planted:
            continue
        gyro = [c["gyro"] for c in planted]
        rob = solver.solve_host([to_step(c["cams"]) for c in planted], gyro, robust=True)
        assert [[int(m) for m in r["rejected"][:k]] for r in rob] == [c["planted"] for c in planted] and rob["fused"]["valid"].all()
        for planar, gs in ((False, 0.0), (True, GYRO_SIGMA)):
            prm = RefineParams(planar=planar, gyro_sigma=gs, z=float(rob["fused"]["pos"][0, 2]))
            masked = solver.refine_host([to_step(c["cams"]) for c in planted], gyro, rob, prm)
            deleted = solver.refine_host([to_step(NR.delete_planted(c)) for c in planted], gyro, rob["fused"], prm)
            assert masked.tobytes() == deleted.tobytes() and (planar or (masked["status"] <= A.CK_RIG_REFINE_MAXITERS).all())
            assert (masked["n_points"] == 4 * rob["fused"]["n_tags"]).all()
            n += len(planted)
    assert n >= 12


def test_frozen_behaviour(solver):
    R_t, p_t = F.truth_pose()
    cams = F.render(F.SCENES["near_far"], np.random.default_rng(3), F.NOISE)
    step = to_step(cams)
    st = start_record(R_t, p_t)
    # no start: NO_START and nothing else
    none = np.zeros(1, RESULT_DTYPE)
    r = solver.refine_host([step], [0.1], none)[0]
    want = np.zeros(1, REFINED_DTYPE)
    want["status"] = A.CK_RIG_REFINE_NO_START
    assert r.tobytes() == want.tobytes()
    # every tag rejected, and an instant without tags: DEGENERATE with the start's pose, no covariance
    rej = np.zeros((1, A.CK_RIG_MAX_CAMS), np.uint64)
    rej[0, 0] = 3
    out = np.zeros(1, REFINED_DTYPE)
    n_cams, probs, tarr, nt, barr = pack_steps([step])
    prm = RefineParams()._c(solver._L)
    assert solver._L.ck_rig_refine_host(C.byref(prm), n_cams, probs, 1, tarr, nt, barr.ctypes.data, len(barr), None, st.ctypes.data,
                                        rej.ctypes.data, out.ctypes.data_as(C.POINTER(A.RigRefined))) == A.CK_OK
    empty = solver.refine_host([[([], np.zeros((0, 3)), step[0][2])]], None, st)
    for r in (out[0], empty[0]):
        assert r["status"] == A.CK_RIG_REFINE_DEGENERATE and r["n_points"] == 0 and r["iters"] == 0
        assert np.array_equal(r["rot"], R_t) and np.array_equal(r["pos"], p_t) and not r["cov"].any() and not r["std_devs"].any()
    # one tag exactly on the optical axis of its camera, six unknowns
    Am, bb = F.mount(F.FRONT, (0, 0, 0.5))
    axis = [((Am, bb), [(R_t @ F.FACING_MINUS_X, tuple(p_t + R_t @ np.array([3.0, 0.0, 0.5]))), (F.FACING_MINUS_X, (4.5, 1.5, 0.9))])]
    cams = F.render(axis)
    assert np.abs(cams[0][1][:4].mean(axis=0) / np.linalg.norm(cams[0][1][:4].mean(axis=0)) - [0, 0, 1]).max() < 1e-12
    st2 = start_record(F.exp_so3(np.array([0.002, 0.001, -0.004])) @ R_t, p_t + 0.01)
    r = solver.refine_host([to_step(cams)], None, st2, RefineParams(max_iters=100))[0]
    assert r["status"] == A.CK_RIG_REFINE_CONVERGED and np.abs(r["pos"] - p_t).max() < 1e-11 and np.isfinite(r["cov"]).all()
    # the same call twice: the same bytes
    a = solver.refine_host([step], [0.1], st, RefineParams(planar=True, gyro_sigma=GYRO_SIGMA))
    assert a.tobytes() == solver.refine_host([step], [0.1], st, RefineParams(planar=True, gyro_sigma=GYRO_SIGMA)).tobytes()


def misuse(call, solver):
    """the refusals both stand-alone entry points share, in the order the header states; call(params, n_cams, probs, n, tarr, nt, barr,
    nb, gyro, start, out) -> rc, with None for a null pointer"""
    cams = F.render(F.SCENES["near_far"], np.random.default_rng(5), F.NOISE)
    n_cams, probs, tarr, nt, barr = pack_steps([to_step(cams)])
    g = np.array([0.1])
    st = start_record(*F.truth_pose())
    L = solver._L

    def prm(**kw):
        p = A.RigRefineParams()
        L.ck_rig_refine_params_default(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    d = prm()
    assert (d.mode, d.max_iters, d.sigma_rad, d.gyro_sigma_rad, d.z) == (A.CK_RIG_REFINE_FREE, 10, 1e-3, 0.0, 0.0)
    out = np.zeros(1, REFINED_DTYPE)
    assert call(d, n_cams, probs, 1, tarr, nt, barr, len(barr), None, st, out) == A.CK_OK and out["status"][0] == A.CK_RIG_REFINE_CONVERGED
    out.view(np.uint8)[:] = 0x5A
    keep = out.tobytes()
    nan, inf = float("nan"), float("inf")
    bad_params = ({"mode": 2}, {"mode": -1}, {"sigma_rad": 0.0}, {"sigma_rad": -1e-3}, {"sigma_rad": nan}, {"sigma_rad": inf}, {"z": nan}, {"z": inf},
                  {"gyro_sigma_rad": -0.01}, {"gyro_sigma_rad": nan}, {"gyro_sigma_rad": inf}, {"max_iters": 0}, {"max_iters": 101})
    for kw in bad_params:
        assert call(prm(**kw), n_cams, probs, 1, tarr, nt, barr, len(barr), g, st, out) == A.CK_EINVAL, kw
        assert call(prm(**kw), n_cams, probs, 0, tarr, nt, barr, len(barr), g, st, out) == A.CK_EINVAL, kw
    assert call(prm(gyro_sigma_rad=0.01), n_cams, probs, 1, tarr, nt, barr, len(barr), None, st, out) == A.CK_EINVAL
    assert call(prm(gyro_sigma_rad=0.01), n_cams, probs, 1, tarr, nt, barr, len(barr), g, st, out) == A.CK_OK
    out.view(np.uint8)[:] = 0x5A
    # null pointers come first, the records' checks second: each is refused whatever the parameters say
    for p in (d, prm(mode=7)):
        assert call(p, n_cams, None, 1, tarr, nt, barr, len(barr), g, st, out) == A.CK_EINVAL
        assert call(p, n_cams, probs, 1, tarr, nt, barr, len(barr), g, None, out) == A.CK_EINVAL
        assert call(p, n_cams, probs, 1, tarr, nt, barr, len(barr), g, st, None) == A.CK_EINVAL
        assert call(p, 0, probs, 1, tarr, nt, barr, len(barr), g, st, out) == A.CK_EINVAL
        assert call(p, 9, probs, 1, tarr, nt, barr, len(barr), g, st, out) == A.CK_EINVAL
        assert call(p, n_cams, probs, -1, tarr, nt, barr, len(barr), g, st, out) == A.CK_EINVAL
        assert call(p, n_cams, probs, 1, None, nt, barr, len(barr), g, st, out) == A.CK_EINVAL
        assert call(p, n_cams, probs, 1, tarr, nt, None, len(barr), g, st, out) == A.CK_EINVAL
        assert call(p, n_cams, probs, 1, tarr, nt - 1, barr, len(barr), g, st, out) == A.CK_EINVAL
        keep_nb = probs[0].n_bearings
        probs[0].n_bearings = keep_nb - 1
        assert call(p, n_cams, probs, 1, tarr, nt, barr, len(barr), g, st, out) == A.CK_EINVAL
        probs[0].n_bearings = keep_nb
    assert call(None, n_cams, probs, 1, tarr, nt, barr, len(barr), g, st, out) == A.CK_EINVAL
    assert out.tobytes() == keep                                                      # nothing was written by any refusal


def test_misuse(solver):
    L = solver._L

    def call(p, n_cams, probs, n, tarr, nt, barr, nb, g, st, out):
        return L.ck_rig_refine_host(None if p is None else C.byref(p), n_cams, probs, n, tarr, nt, None if barr is None else barr.ctypes.data, nb,
                                    None if g is None else g.ctypes.data, None if st is None else st.ctypes.data, None,
                                    None if out is None else out.ctypes.data_as(C.POINTER(A.RigRefined)))
    misuse(call, solver)
    with pytest.raises(TypeError):
        solver.refine_host([], [], np.zeros(0, RESULT_DTYPE), refine=1.5)
    assert len(solver.refine_host([], [], np.zeros(0, RESULT_DTYPE))) == 0


def test_refine_kernel_uses_no_private_segment_and_no_lds(built):
    """k_rig_refine keeps its per-lane arrays in registers and its point records in the call's workspace: the gfx950 code object's
    metadata shows a private segment of 0 bytes, no spilled vector register and no LDS (read as tests/test_rig_robust_host.py reads
    k_rig_robust's)."""
    import shutil
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    res = {}
    with tempfile.TemporaryDirectory() as td:
        obj = "k_rig_refine.o"
        shutil.copy(os.path.join(ROOT, "chalkydri_amd", "csrc", "build", obj), td)
        subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", obj], cwd=td, stdout=subprocess.DEVNULL)
        co = [f for f in os.listdir(td) if f.startswith(obj) and "amdgcn" in f][0]
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], cwd=td, text=True)
        name, lds = None, None
        for line in notes.splitlines():
            m = re.match(r"[\s-]*\.group_segment_fixed_size:\s+(\d+)", line)    # (the keys of a kernel are sorted: this one precedes .name)
            if m:
                lds = int(m.group(1))
            m = re.match(r"\s*\.name:\s+(\S+)", line)
            if m:
                name = m.group(1)
                res[name] = {"group_segment_fixed_size": lds}
            m = re.match(r"\s*\.(vgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)", line)
            if m and name:
                res[name][m.group(1)] = int(m.group(2))
    kernels = [v for k, v in res.items() if "k_rig_refine" in k]
    print(res)
    assert len(kernels) == 1
    v = kernels[0]
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["group_segment_fixed_size"] == 0, v


def test_host_twin_under_sanitizers(built):
    """tests/cpp/rig_refine_asan.c, a stand-alone program of the twin's C files built with -fsanitize=address,undefined, over the shapes at
    which the walkers' loops end differently; it exits non-zero on the first finding of either sanitizer"""
    sym = subprocess.run(["nm", ASAN], capture_output=True, text=True).stdout
    assert "__asan_init" in sym and "__ubsan_handle" in sym          # the build that ran is the sanitized one
    r = subprocess.run([ASAN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
