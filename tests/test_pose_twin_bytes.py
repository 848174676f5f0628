"""The rig solver's host twin (ck_rig_solve_host, ck_rig_solve_robust_host) against what it returned when
tests/golden/pose_twin_golden.json was written (tests/golden/make_pose_twin_golden.py).  tests/test_gpu_rig.py holds k_rig to the twin
to 1e-9, so a change that moves both together, or either by less than that, passes there; this test holds the twin where it was.  The
fixture stores the inputs themselves.

valid, n_tags, cam_tags, energy, cam_rms, std_devs (and the robust record's own fields) come from + - * / sqrt alone, -ffp-contract=off:
byte for byte.  rot, pos, yaw pass through the C library's atan2 / fmod / cos / sin / asin in the yaw pivot, which may differ in the last
bit between machines: TOL, the bound of tests/test_gpu_rig.py for the same cause.  (cos / sin of the heading enter the candidates'
penalty too, but only the choice among them depends on it.)"""
import base64
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

from chalkydri_amd import _abi as A
from chalkydri_amd.rig import RESULT_DTYPE, ROBUST_RESULT_DTYPE, RigSolver, RobustParams

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "pose_twin_golden.json")))
BLOB = zlib.decompress(base64.b64decode(GOLDEN["blob"]))
TOL = 1e-9
DBL_MAX = float(np.finfo(np.float64).max)
EXACT = ("valid", "n_tags", "cam_tags", "energy", "cam_rms", "std_devs")
LIBM = ("rot", "pos", "yaw")


def raw(at):
    return BLOB[at[0]:at[0] + at[1]]


def isos(at):
    b = raw(at)
    return [A.Iso3.from_buffer_copy(b[i:i + C.sizeof(A.Iso3)]) for i in range(0, len(b), C.sizeof(A.Iso3))]


def step_of(g):
    tags, bear, mounts, at, cams = isos(g["tags"]), np.frombuffer(raw(g["bearings"]), np.float64).reshape(-1, 3), isos(g["mounts"]), 0, []
    for n, m in zip(g["counts"], mounts):
        cams.append((tags[at:at + n], bear[4 * at:4 * (at + n)].copy(), m))
        at += n
    return cams, float(np.frombuffer(raw(g["gyro"]), np.float64)[0])


def same_fused(name, got, want):
    for k in EXACT:
        assert got[k].tobytes() == want[k].tobytes(), (name, k, got[k], want[k])
    for k in LIBM:
        assert np.abs(got[k] - want[k]).max() < TOL, (name, k, got[k], want[k])
    print(name, "every byte equal" if got.tobytes() == want.tobytes() else "rot / pos / yaw differ in their last bits")


@pytest.mark.parametrize("g", GOLDEN["plain"], ids=[g["name"] for g in GOLDEN["plain"]])
def test_rig_twin(built, g):
    step, gyro = step_of(g)
    got = RigSolver().solve_host([step], [gyro])[0]
    want = np.frombuffer(raw(g["result"]), RESULT_DTYPE)[0]
    name, tags = g["name"], list(got["cam_tags"][:len(step)])
    if name == "no-tag":                                                   # the paths, from the twin's own output
        assert got.tobytes() == bytes(got.nbytes)
    else:
        assert got["valid"] == 1 and tags == g["counts"]
    if name == "three-beside-none":
        assert tags == [3, 0]
    if name == "one-tag":                                                  # four corners of one tag: coplanar
        assert tags == [1]
    assert all(v == DBL_MAX for v in got["std_devs"]) == (name == "untrusted-rms")
    same_fused(name, got, want)


@pytest.mark.parametrize("g", GOLDEN["robust"], ids=[g["name"] for g in GOLDEN["robust"]])
def test_rig_robust_twin(built, g):
    """The paths: "clean" passes the gate, no round.  "wrong-tag" ends settled, the planted tag at weight 0.  A round runs only when
    the worst tag's rho_max > c^2, and with the first round's mu = c^2 / (2 rho_max - c^2) the weight is 1 up to c^4 / (2 rho_max) <
    c^2 and 0 from 2 rho_max on: that tag's first weight lies inside (0, 1) whenever rounds >= 1.  "out-of-rounds" stops one round
    before the weights of "wrong-tag" settle: the inliers by w >= 0.5."""
    step, gyro = step_of(g)
    got = RigSolver().solve_host([step], [gyro], robust=RobustParams(max_rounds=g["max_rounds"]))[0]
    want = np.frombuffer(raw(g["result"]), ROBUST_RESULT_DTYPE)[0]
    name, rejected = g["name"], [int(m) for m in got["rejected"][:len(step)]]
    if name == "clean":
        assert (got["status"], got["rounds"], got["n_rejected"]) == (A.CK_RIG_ROBUST_CLEAN, 0, 0) and not any(rejected)
    elif name == "wrong-tag":
        assert got["status"] == A.CK_RIG_ROBUST_REJECTED and 1 <= got["rounds"] < g["max_rounds"] and rejected == g["planted"]
    else:
        assert got["status"] == A.CK_RIG_ROBUST_MAXROUNDS and got["rounds"] == g["max_rounds"] >= 1
    for k in ("status", "rounds", "n_rejected", "pad", "rejected", "worst_inlier_rad", "best_rejected_rad"):
        assert got[k].tobytes() == want[k].tobytes(), (name, k, got[k], want[k])
    same_fused(name, got["fused"], want["fused"])
