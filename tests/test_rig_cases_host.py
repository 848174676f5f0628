"""The cases of tests/rig_cases.py reach the edges they are named for (asserted on the read-out of the numpy restatement, `trace` of
np_rig.solve_rig and np_rig_robust.solve_robust), their discrete results survive a perturbation of 2^-50, and the host twin
(ck_rig_solve_host, ck_rig_solve_robust_host) agrees with the restatement on every one of them.  No GPU is needed;
tests/test_gpu_rig_cases.py runs the same cases on the device.

What was reached (figures of the read-out; kappa is the largest change of a continuous result under the perturbation, over the case's
steps, and the bound max(1e-9, 64 kappa); every step of every case is stable, none is exempt):

    case                      what the read-out shows                                                                kappa    bound
    count_one_camera          60, 64, 68, 124, 128, 132, 256 points in one camera; winner 0                          3.0e-13  1e-9
    count_one_camera_robust   the same with a wrong id in the last tag: masks 1 << 14, 15, 16, 30, 31, 32, 63,      4.6e-13  1e-9
                              16..20 rounds; a clean step of 64 tags (rho_max 0.04 gate^2, no round)
    count_bit63               2 x 64 tags, 512 points                                                                2.9e-14  1e-9
    count_bit63_robust        masks 0x8000000000000000 and 0x8000000000000001 (global tags 63, 64, 127), 16 rounds;  3.7e-14  1e-9
                              the clean step CLEAN
    count_full                8 x 64 = 2048 points and 8 x 65 = 2080 points                                          9.5e-15  1e-9
    count_full_robust         global tags 0, 63, 64, 127, 128, 255, 256, 511 rejected and no other, 22 rounds;       7.4e-15  1e-9
                              the clean 512 tags CLEAN
    count_eight_by_five       128 and 160 points over 8 cameras                                                      3.5e-13  1e-9
    count_eight_by_five_robust  masks (7: 0x8) and (0: 0x1, 4: 0x10), 18 rounds each; the clean steps CLEAN          2.3e-13  1e-9
    cams_sparse               tags in cameras (7), (0, 7), (3, 4), (1..7), (1, 3, 5, 7) of 8                         7.6e-13  1e-9
    planar_wall               6, 6, 1, 2, 1 tags, all coplanar: scatter ratio wmin / wmax within +-1e-16            1.3e-12  1e-9
    planar_near               lift 1e-9, 1e-7 m: coplanar (ratio -2.5e-16, 3.2e-15); 1e-5, 1e-3, 1e-1 m: free        4.9e-9   3.1e-7
                              (3.3e-11, 3.3e-7, 3.2e-3); kappa 4.9e-9 at 1e-5 m, at most 3.8e-13 elsewhere
    free_3d                   scatter ratio 0.036, 0.028: free                                                       2.6e-13  1e-9
    singular_qtt              det(Q_tt) = 0.0 exactly (1 and 2 tags); no candidate in front, no pose (twin-only)     0        1e-9
    far_and_near              tags 0.30 .. 42.8 m from their camera, a mount 2.47 m from the robot's origin          1.4e-12  1e-9
    cheirality_second         seeds 1, 2, 3: winner 3 of 6, the three cheaper candidates all behind the camera       1.4e-12  1e-9
                              (penalised 1.5, 52.4, 663.8 against the winner's 849.1, 792.9, 1081.4); yaw weight 1
    cheirality_none           seed 0: all six candidates behind a camera (cheapest penalised 0.0215; 0.029 with the  4.4e-13  1e-9
                              points behind at 64..67, beyond rig_pick's first stride); the neighbours solved
    gyro_sweep_a              weights 8e-7, 0.2586, 0.999955, 0.999999, 1, 1, 1, 1; winner 0 x 6, then 4, 4: at     7.7e-13  1e-9
                              179 and 180 deg four cheaper candidates lose to cheirality, the penalty sets the order
    gyro_sweep_b              weights 0.26, 0.999976, 1, 1, 1, 1; winner 4 at -90 and -179 deg; across the wrap      7.3e-13  1e-9
                              delta +0.1493 and -0.1489 where gyro - vision_yaw is beyond -+pi
    std_branches              rms 8e-15, 0.002, 0.03, 0.09, 0.11: (xy, th) = (lo, lo), (mid, mid), (mid, hi),        1.8e-11  1.2e-9
                              (hi, hi), untrusted (DBL_MAX)
    gate_edge                 rho_max / gate^2 = 0.95: CLEAN, no round; 1.05: 9 rounds, the tag at the gate dropped  1.1e-12  1e-9
    all_outliers              seeds 12, 20, 25, 0: every weight 0 after 2, 11, 13, 3 rounds, NO_CONSENSUS; the last  0        1e-9
                              also without a candidate in front on the first pass
    first_pass_not_found      seed 0: no candidate in front on the first pass (also with the impossible tag at       5.0e-13  1e-9
                              points 64..67), the impossible tag dropped in 17 rounds, a pose of the rest

Not built: a scene made for svd3's rank-2 completion (polar_rotation's determinant flip needs none: one start of every +- pair has a
negative determinant, so every solve takes it).  The restatement has no separate read-out for either; both are leaf arithmetic of
ck_pose_math.h that the comparison against the restatement judges through the record.

singular_qtt is judged against the twin only, as its name says: the restatement tests abs(det) > 0 on a LAPACK determinant and need
not agree with mat3_try_inverse's cofactor determinant.  On these two steps it does agree (both determinants are exactly 0, both
sides zero Q_tt^-1, no candidate is in front of the camera, no pose)."""
import numpy as np
import pytest

import np_rig as N
import np_rig_robust as NR
import rig_cases as rc

from chalkydri_amd.rig import RigSolver


def _points(cams):
    return 4 * sum(len(t) for t, _, _ in cams)


def _fused(step):
    return step["trace"].get("fused", step["trace"])


def _masks_are_planted(c, r):
    for i, (step, planted) in enumerate(zip(r, c["planted"])):
        if planted is None:
            continue
        ref = step["ref"]
        assert list(ref["rejected"]) == planted, (c["name"], i, ref["rejected"], planted)
        assert ref["status"] == (NR.REJECTED if any(planted) else NR.CLEAN) and (ref["rounds"] > 0) == any(planted)


def reached(name):
    """asserts that the case reaches what it is named for; returns the figures for the table"""
    c, r = rc.case(name), rc.restated(name)
    base = name[:-len("_robust")] if name.endswith("_robust") else name
    pts = [_points(s) for s in c["steps"]]
    if c["robust"] is not None:
        _masks_are_planted(c, r)
    if base == "count_one_camera":
        assert pts[:7] == [60, 64, 68, 124, 128, 132, 256]
        if c["robust"] is not None:
            assert [s["ref"]["rejected"][0] for s in r] == [1 << 14, 1 << 15, 1 << 16, 1 << 30, 1 << 31, 1 << 32, 1 << 63, 0] and pts[7] == 256
        return {"points": pts}
    if base == "count_bit63":
        if c["robust"] is not None:
            assert r[0]["ref"]["rejected"] == [1 << 63, 1 | 1 << 63] and r[1]["ref"]["status"] == NR.CLEAN
        assert pts[0] == 512 and all(len(t) == 64 for t, _, _ in c["steps"][0])
        return {"points": pts, "masks": None if c["robust"] is None else [hex(m) for m in r[0]["ref"]["rejected"]]}
    if base == "count_full":
        assert pts[0] == 2048 and (c["robust"] is not None or pts[1] == 2080)
        if c["robust"] is not None:
            keep = r[0]["ref"]["keep"]
            assert list(np.flatnonzero(~keep)) == [0, 63, 64, 127, 128, 255, 256, 511] and r[1]["ref"]["status"] == NR.CLEAN and pts[1] == 2048
        return {"points": pts, "rounds": None if c["robust"] is None else r[0]["ref"]["rounds"]}
    if base == "count_eight_by_five":
        sizes = sorted(set(pts))
        assert sizes == [128, 160] and all(len(t) > 0 for s in c["steps"] for t, _, _ in s)
        return {"points": pts}
    if name == "cams_sparse":
        seen = [tuple(k for k, (t, _, _) in enumerate(s) if len(t)) for s in c["steps"]]
        assert seen == [(7,), (0, 7), (3, 4), (1, 2, 3, 4, 5, 6, 7), (1, 3, 5, 7)] and all(s["ref"] is not None for s in r)
        return {"cameras with tags": seen}
    if name == "planar_wall":
        assert all(s["trace"]["coplanar"] and s["ref"] is not None for s in r)
        assert [_points(s) // 4 for s in c["steps"]] == [6, 6, 1, 2, 1]
        return {"scatter ratio": [s["trace"]["planar_ratio"] for s in r]}
    if name == "planar_near":
        flags = [s["trace"]["coplanar"] for s in r]
        assert True in flags and False in flags and flags == sorted(flags, reverse=True)
        return {"lift": c["lifts"], "coplanar": flags, "scatter ratio": [float("%.2g" % s["trace"]["planar_ratio"]) for s in r]}
    if name == "free_3d":
        assert not any(s["trace"]["coplanar"] for s in r) and all(s["trace"]["planar_ratio"] > 1e-3 for s in r)
        return {"scatter ratio": [round(s["trace"]["planar_ratio"], 4) for s in r]}
    if name == "singular_qtt":
        dets = []
        for cams in c["steps"]:
            sys_ = N.System(cams)
            dets.append(float(np.linalg.det(sum(sys_.M))))
            assert dets[-1] == 0.0 and not sys_.Q_tt_inv.any()
        assert all(s["ref"] is None for s in r)
        return {"det(Q_tt)": dets, "pose": [s["ref"] is not None for s in r]}
    if name == "far_and_near":
        figs = []
        for cams, s in zip(c["steps"], r):
            ref = s["ref"]
            d = [np.linalg.norm(t - (ref["rot"] @ (-A.T @ b) + ref["pos"])) for tags, _, (A, b) in cams for _, t in tags]
            off = max(np.linalg.norm(A.T @ b) for _, _, (A, b) in cams)
            assert min(d) < 0.4 and max(d) > 39.0 and off > 1.0
            figs.append((round(min(d), 2), round(max(d), 1), round(off, 2)))
        return {"nearest, farthest tag, largest mount offset (m)": figs}
    if name == "cheirality_second":
        for s in r:
            t = s["trace"]
            assert t["winner"] > 0 and not any(k["in_front"] for k in t["candidates"][:t["winner"]])
            assert t["candidates"][0]["penalised"] < t["candidates"][t["winner"]]["penalised"] and t["yaw_weight"] == 1.0
        return {"seeds": rc.CHEIRALITY_SECOND_SEEDS, "winner": [s["trace"]["winner"] for s in r],
                "penalised (cheapest, winner)": [(round(s["trace"]["candidates"][0]["penalised"], 1),
                                                 round(s["trace"]["candidates"][s["trace"]["winner"]]["penalised"], 1)) for s in r]}
    if name == "cheirality_none":
        assert [s["ref"] is None for s in r] == [False, True, False, True]
        for i in (1, 3):
            assert r[i]["trace"]["winner"] is None and not any(k["in_front"] for k in r[i]["trace"]["candidates"])
        assert len(c["steps"][3][0][0]) == 16                     # the points behind their camera are 64..67
        return {"seed": rc.CHEIRALITY_NONE_SEED, "cheapest penalised": [round(r[i]["trace"]["candidates"][0]["penalised"], 4) for i in (1, 3)]}
    if name == "gyro_sweep_a":
        w = [s["trace"]["yaw_weight"] for s in r]
        assert w[0] < 1e-4 and 0.2 < w[1] < 0.3 and w[2] < 1.0 and w[4:] == [1.0] * 4 and all(s["trace"]["yaw_delta"] >= -1e-3 or i >= 6 for i, s in enumerate(r))
        win = [s["trace"]["winner"] for s in r]
        assert win[0] == 0 and max(win) > 0                       # the penalty decides the order
        return {"weight": [float("%.6g" % x) for x in w], "winner": win}
    if name == "gyro_sweep_b":
        w = [s["trace"]["yaw_weight"] for s in r]
        assert 0.2 < w[0] < 0.3 and w[1] < 1.0 and w[3:6] == [1.0] * 3 and all(s["trace"]["yaw_delta"] < 0 for s in r[:6])
        for s, g, sign in zip(r[6:], c["gyro"][6:], (1, -1)):     # the wrap: gyro - vision_yaw is beyond +-pi, the delta small and of the other sign
            t = s["trace"]
            assert abs(g - t["vision_yaw"]) > np.pi and abs(t["yaw_delta"]) < 0.2 and np.sign(t["yaw_delta"]) == sign == -np.sign(g - t["vision_yaw"])
        win = [s["trace"]["winner"] for s in r]
        assert max(win) > 0
        return {"weight": [float("%.6g" % x) for x in w], "winner": win, "wrapped delta": [round(s["trace"]["yaw_delta"], 4) for s in r[6:]]}
    if name == "std_branches":
        br = [s["trace"]["std_branch"] for s in r]
        assert br == [("lo", "lo"), ("mid", "mid"), ("mid", "hi"), ("hi", "hi"), ("untrusted",)]
        rms = [s["trace"]["rms"] for s in r]
        assert 0.085 < rms[3] < 0.095 and 0.105 < rms[4] < 0.115
        assert np.all(r[4]["ref"]["std"] == rc.DBL_MAX) and r[3]["ref"]["std"][0] == 10.0 and r[3]["ref"]["std"][2] == np.pi
        assert r[2]["ref"]["std"][2] == np.pi and 0.01 < r[2]["ref"]["std"][0] < 10.0 and list(r[0]["ref"]["std"]) == [0.01, 0.01, 0.05]
        return {"rms": [float("%.4g" % x) for x in rms], "branches (xy, th)": br}
    if name == "gate_edge":
        g = [s["trace"]["gate_ratio"] for s in r]
        assert 0.9 < g[0] < 1.0 < g[1] < 1.1
        assert (r[0]["ref"]["status"], r[0]["ref"]["rounds"]) == (NR.CLEAN, 0) and r[1]["ref"]["rounds"] > 0
        return {"rho_max / gate^2": [round(x, 6) for x in g], "status": [s["ref"]["status"] for s in r], "rounds": [s["ref"]["rounds"] for s in r],
                "masks": [s["ref"]["rejected"] for s in r]}
    if name == "all_outliers":
        for s in r:
            assert not s["trace"]["alive"] and s["ref"]["status"] == NR.NO_CONSENSUS and s["ref"]["fused"] is None and not s["ref"]["keep"].any()
        assert [s["trace"]["found"] for s in r] == [True, True, True, False]
        return {"seeds": rc.ALL_OUTLIERS_SEEDS, "rounds": [s["ref"]["rounds"] for s in r]}
    if name == "first_pass_not_found":
        assert [s["trace"]["found"] for s in r] == [False, True, False]
        assert all(s["ref"]["fused"] is not None for s in r) and len(c["steps"][2][0][0]) == 16
        return {"seed": rc.FIRST_PASS_SEED, "rounds": [s["ref"]["rounds"] for s in r], "masks": [s["ref"]["rejected"] for s in r]}
    raise KeyError(name)


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_reaches_its_edge(name):
    c = rc.case(name)
    assert len(c["steps"]) <= 8 and max(_points(s) for s in c["steps"]) <= (2048 if c["robust"] is not None else 2080)
    figures = reached(name)
    r = rc.restated(name)
    print(name, figures, "| kappa %.1e bound %.1e" % (max(s["kappa"] for s in r), max(s["bound"] for s in r)))


@pytest.mark.parametrize("name", rc.NAMES)
def test_discrete_results_are_stable(name):
    """validity, the coplanar flag, the winner, the branches of the standard deviations, the inlier masks, the status and the rounds
    are the same on the inputs and on 8 copies perturbed by 2^-50: no step is exempt (singular_qtt, twin-only by its name, passes as
    well); and no step is too ill-conditioned to judge anything (bound <= 1e-6)."""
    for i, s in enumerate(rc.restated(name)):
        assert s["stable"], (name, i, s["discrete"])
        assert s["bound"] <= 1e-6, (name, i, s["kappa"])


@pytest.fixture(scope="module")
def host(built):
    return RigSolver()


@pytest.mark.parametrize("name", rc.NAMES)
def test_twin_matches_restatement(host, name):
    """discrete fields equal, continuous ones within max(1e-9, 64 kappa) of the step, DBL_MAX standard deviations equal; a step
    without a pose is an all-zero record.  (singular_qtt is twin-only; it is compared all the same, and agrees.)"""
    c = rc.case(name)
    got = rc.solve(host, c, host=True)
    worst = 0.0
    for i, (g, s) in enumerate(zip(got, rc.restated(name))):
        worst = max(worst, rc.against_restatement(f"{name}[{i}] twin vs restatement", c, g, s))
    print(name, "twin vs restatement: worst", worst)


def test_twin_refuses_65_tags_robust(host):
    """the 8 x 65 step of count_full: the plain twin solves it, the robust one refuses it"""
    from chalkydri_amd import _abi as A
    from chalkydri_amd._lib import ChalkydriError
    c = rc.case("count_full")
    steps, gyro = [rc.to_step(c["steps"][1])], [c["gyro"][1]]
    assert host.solve_host(steps, gyro)[0]["valid"] == 1
    with pytest.raises(ChalkydriError) as e:
        host.solve_host(steps, gyro, robust=True)
    assert e.value.code == A.CK_EINVAL


def test_sparse_cameras_are_the_compacted_step(host):
    """the twin's promise of test_rig_host.test_edge_cases at every pattern of cams_sparse: bytes of the compacted step"""
    c = rc.case("cams_sparse")
    got = rc.solve(host, c, host=True)
    for i, (cams, g) in enumerate(zip(c["steps"], got)):
        small, idx = rc.compact(cams)
        w = host.solve_host([rc.to_step(small)], [c["gyro"][i]])[0]
        rc.same_but_for_the_cameras(f"cams_sparse[{i}]", g, w, idx)


def test_read_out_adds_output_only():
    """with and without `trace` the restatements return the same bits"""
    for name, i in (("planar_wall", 1), ("std_branches", 4), ("cheirality_second", 0)):
        c = rc.case(name)
        a, b = N.solve_rig(c["steps"][i], c["gyro"][i]), N.solve_rig(c["steps"][i], c["gyro"][i], trace={})
        assert a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    c = rc.case("gate_edge")
    a, b = NR.solve_robust(c["steps"][1], c["gyro"][1]), NR.solve_robust(c["steps"][1], c["gyro"][1], trace={})
    assert (a["status"], a["rounds"], a["rejected"], a["worst"], a["best"]) == (b["status"], b["rounds"], b["rejected"], b["worst"], b["best"])
    assert all(np.asarray(a["fused"][k]).tobytes() == np.asarray(b["fused"][k]).tobytes() for k in a["fused"])
