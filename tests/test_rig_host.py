"""The arithmetic of the camera-rig solver on the host (ck_rig_solve_host, chalkydri_amd/csrc/ck_rig_host.c) against
its numpy restatement (tests/np_rig.py), the truth of noise-free rigs, the one-camera oracle and a many-start global minimum.  No
device is needed: the device solver is compared with this twin in tests/test_gpu_rig.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_rig as N  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd.rig import RESULT_DTYPE, RigSolver, pack_steps  # noqa: E402
from chalkydri_amd.sqpnp import iso3  # noqa: E402


def to_step(cams):
    """np_rig cameras -> what RigSolver takes"""
    return [([iso3(t, N.mat_to_quat(R)) for R, t in tags], b, iso3(bb, N.mat_to_quat(Am))) for tags, b, (Am, bb) in cams]


def angle(Ra, Rb):
    return np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))


@pytest.fixture(scope="module")
def rigs():
    """test 1's generator: 200 seeded rigs, 1-4 cameras, 0-3 tags per camera, bearing noise 0 (even) and 1e-3 (odd)"""
    rng = np.random.default_rng(20261019)
    out = []
    for i in range(200):
        noise = 0.0 if i % 2 == 0 else 1e-3
        cams, gyro, truth = N.make_rig(rng, noise=noise, gyro_noise=0.0 if noise == 0.0 else 0.02)
        out.append((cams, gyro, truth, noise))
    return out


@pytest.fixture(scope="module")
def twin(built, rigs):
    """one solve per rig (a step each: the number of cameras differs)"""
    s = RigSolver()
    return [s.solve_host([to_step(cams)], [gyro])[0] for cams, gyro, _, _ in rigs]


def test_twin_matches_restatement(rigs, twin):
    worst = {"rot": 0.0, "pos": 0.0, "yaw": 0.0, "energy": 0.0, "cam_rms": 0.0, "std": 0.0}
    for (cams, gyro, _, _), got in zip(rigs, twin):
        want = N.solve_rig(cams, gyro)
        assert bool(got["valid"]) == (want is not None)
        if want is None:
            assert got.tobytes() == bytes(got.nbytes)
            continue
        assert list(got["cam_tags"][:len(cams)]) == want["cam_tags"] and not got["cam_tags"][len(cams):].any()
        assert got["n_tags"] == want["n_tags"]
        worst["rot"] = max(worst["rot"], np.abs(got["rot"] - want["rot"]).max())
        worst["pos"] = max(worst["pos"], np.abs(got["pos"] - want["pos"]).max())
        worst["yaw"] = max(worst["yaw"], abs(got["yaw"] - want["yaw"]))
        if want["energy"] > 1e-13:       # below that the energy of exact data is round-off (the project's line: test_sqpnp_oracle.py)
            worst["energy"] = max(worst["energy"], abs(got["energy"] - want["energy"]) / want["energy"])
        else:
            assert abs(got["energy"]) < 1e-12
        worst["cam_rms"] = max(worst["cam_rms"], np.abs(got["cam_rms"][:len(cams)] - want["cam_rms"]).max())
        if want["energy"] > 1e-13:
            worst["std"] = max(worst["std"], np.abs(got["std_devs"] - want["std"]).max())
    print("twin vs restatement:", worst)
    assert worst["rot"] < 1e-9 and worst["pos"] < 1e-9 and worst["yaw"] < 1e-9 and worst["energy"] < 1e-9
    assert worst["std"] < 1e-9 and worst["cam_rms"] < 1e-9


def test_noise_free_truth(rigs, twin):
    worst_p = worst_a = 0.0
    count = 0
    for (cams, gyro, truth, noise), got in zip(rigs, twin):
        if noise != 0.0:
            continue
        assert got["valid"]
        count += 1
        worst_p = max(worst_p, np.linalg.norm(got["pos"] - truth["pos"]))
        worst_a = max(worst_a, angle(got["rot"], truth["rot"]))
    print("noise-free:", count, "rigs, worst position", worst_p, "m, worst angle", worst_a, "rad")
    assert count == 100 and worst_p < 1e-6 and worst_a < 1e-6


def test_one_camera_rig_is_sqpnp(oracle):
    """A rig of one camera is today's solver: g = 0 and Omega is SQPnP's in another basis.  50 noisy problems of 2 or 3 tags against
    the oracle's solve_robot_pose: rot and pos within 1e-9 on all of them.  (One tag alone is a coplanar scene: there SQPnP's
    starts are an arbitrary basis of Omega's null space, the oracle's pose depends on that basis, and the rig solver
    takes its starts outside that null space, §4k; test_noise_free_truth covers those.)  std_devs takes distance = |t| of world ->
    ROBOT where the per-camera solver takes world -> CAMERA, so the two are the same number only for a mount without translation:
    the even problems have such a mount (std_devs within 1e-9 of the oracle's); the odd ones a mount within +-0.4 m, where the
    expected value is the oracle's energy and tag count with the restatement's |t|."""
    rng = np.random.default_rng(7)
    s = RigSolver()
    worst = {"rot": 0.0, "pos": 0.0, "std": 0.0}
    for i in range(50):
        cams, gyro, _ = N.make_rig(rng, n_cams=1, noise=1e-3, tags_per_cam=(2, 3), gyro_noise=0.02,
                                   mount_translation=0.0 if i % 2 == 0 else 0.4)
        got = s.solve_host([to_step(cams)], [gyro])[0]
        tags, bearings, mount = cams[0]
        want = oracle.sqpnp_solve(tags, bearings, mount, gyro, 600.0)
        assert got["valid"] and want is not None
        worst["rot"] = max(worst["rot"], np.abs(got["rot"] - want["rot"]).max())
        worst["pos"] = max(worst["pos"], np.abs(got["pos"] - want["pos"]).max())
        std = want["std"]
        if i % 2:
            nt, rms = len(tags), np.sqrt(want["energy"] / (4 * len(tags)))
            assert rms <= 0.1
            m = 1 + np.linalg.norm(N.solve_rig(cams, gyro)["t"]) / N.TAG_SIZE
            xy = np.clip(rms * m / np.sqrt(nt) * 5.0, 0.01, 10.0)
            th = np.clip(rms / N.TAG_SIZE * m / np.sqrt(nt) * 2.0, 0.05, np.pi)
            std = np.array([xy, xy, th])
        worst["std"] = max(worst["std"], np.abs(got["std_devs"] - std).max())
    print("one camera vs oracle:", worst)
    assert worst["rot"] < 1e-9 and worst["pos"] < 1e-9 and worst["std"] < 1e-9


def test_global_minimum(built):
    """SQPnP's six starts reach the global minimum: at max_iter = 100 the twin's solution equals the best of 60 random starts plus
    the truth on 300 noisy rigs (2-3 cameras, bearing noise 2e-3), every one of them.  The record gives rot = Rz(pivot) polar(R)^T
    and not r itself, so the reference's r goes through the same last stage (np_rig.finish) and the nine entries are compared."""
    rng = np.random.default_rng(99)
    s = RigSolver().max_iter(100)
    worst = 0.0
    for i in range(300):
        cams, gyro, truth = N.make_rig(rng, n_cams=int(rng.integers(2, 4)), noise=2e-3, tags_per_cam=(1, 2), gyro_noise=0.02)
        got = s.solve_host([to_step(cams)], [gyro])[0]
        want = N.many_start_reference(cams, gyro, truth["R"], rng)
        assert got["valid"] and want is not None, i
        worst = max(worst, np.abs(got["rot"] - want["rot"]).max())
    print("six starts vs 61 starts: worst |d rot|", worst)
    assert worst < 1e-7


def test_edge_cases(built):
    L = RigSolver()._L
    rng = np.random.default_rng(5)
    cams, gyro, _ = N.make_rig(rng, n_cams=3, noise=1e-3, tags_per_cam=(1, 2))
    step = to_step(cams)
    prm = RigSolver().params

    def call(n_cams, probs, n, tarr, nt, barr, g, res=None):
        res = np.zeros(max(n, 1), RESULT_DTYPE) if res is None else res
        return L.ck_rig_solve_host(C.byref(prm), n_cams, probs, n, tarr, nt, barr.ctypes.data, len(barr), g.ctypes.data,
                                   res.ctypes.data_as(C.POINTER(A.RigResult))), res

    n_cams, probs, tarr, nt, barr = pack_steps([step])
    g = np.array([gyro])
    assert call(n_cams, probs, 1, tarr, nt, barr, g)[0] == A.CK_OK
    assert call(0, probs, 1, tarr, nt, barr, g)[0] == A.CK_EINVAL
    assert call(9, probs, 1, tarr, nt, barr, g)[0] == A.CK_EINVAL
    assert L.ck_rig_solve_host(None, n_cams, probs, 1, tarr, nt, barr.ctypes.data, len(barr), g.ctypes.data, None) == A.CK_EINVAL
    for field, value in (("n_bearings", probs[0].n_bearings - 1), ("n_tags", probs[0].n_tags + 1), ("tag_offset", nt), ("bearing_offset", -1),
                         ("bearing_offset", len(barr) - 1), ("n_tags", -1)):
        keep = getattr(probs[0], field)
        setattr(probs[0], field, value)
        assert call(n_cams, probs, 1, tarr, nt, barr, g)[0] == A.CK_EINVAL, field
        setattr(probs[0], field, keep)
    assert call(n_cams, probs, 1, tarr, nt - 1, barr, g)[0] == A.CK_EINVAL          # arrays shorter than the records say
    # a step without tags: valid = 0, an all-zero record, and its neighbour is solved
    empty = [([], np.zeros((0, 3)), m) for _, _, m in step]
    s = RigSolver()
    res = s.solve_host([step, empty], [gyro, gyro])
    assert res[0]["valid"] == 1 and res[1].tobytes() == bytes(res[1].nbytes)
    # a camera without tags does not change the others' result
    base = s.solve_host([step], [gyro])[0]
    more = s.solve_host([step + [([], np.zeros((0, 3)), step[0][2])]], [gyro])[0]
    assert more.tobytes() == base.tobytes()
    first = s.solve_host([[([], np.zeros((0, 3)), step[0][2])] + step], [gyro])[0]
    for k in ("rot", "pos", "std_devs", "yaw", "energy", "n_tags"):
        assert first[k].tobytes() == base[k].tobytes(), k
    assert list(first["cam_tags"][:4]) == [0] + list(base["cam_tags"][:3]) and first["cam_rms"][1:4].tobytes() == base["cam_rms"][:3].tobytes()
    # the order of the cameras only changes the order of the sums
    for perm in ((2, 0, 1), (1, 2, 0), (2, 1, 0)):
        p = s.solve_host([[step[k] for k in perm]], [gyro])[0]
        assert np.abs(p["rot"] - base["rot"]).max() < 1e-9 and np.abs(p["pos"] - base["pos"]).max() < 1e-9
        assert list(p["cam_tags"][:3]) == [base["cam_tags"][k] for k in perm]
