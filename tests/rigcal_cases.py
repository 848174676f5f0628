"""What the mount calibration tests share: the conversion of np_rigcal's scenes to the C ABI's records, the
acceptance captures of the CPU tests and the small shape cases of the GPU tests."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_rigcal as N  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402


def iso(R, t):
    return A.Iso3((C.c_double * 3)(*t), (C.c_double * 4)(*N.mat_to_quat(R)))


def mount_iso(m):
    """(A, o) -> robot_to_cam (A, b = -A o)"""
    return iso(m[0], -m[0] @ m[1])


def mount_of(K, rec):
    """robot_to_cam record of a result -> (A, o)"""
    Am, b = K.iso_matrix(rec)
    return Am, -Am.T @ b


def c_steps(steps):
    """np_rigcal's steps -> what rigcal.Capture takes"""
    return [[([iso(R, t) for R, t in tg], b) for tg, b in cams] for cams in steps]


def pose12(poses):
    return np.array([np.concatenate([R.reshape(9), t]) for R, t in poses]).reshape(-1, 12)


def acceptance_case(n_cams, n_steps, seed, noise):
    """One acceptance input of tests/test_rigcal_host.py: a room capture, the start mounts off by up to 5 degrees and 5 cm (camera 0,
    the gauge, stays), the start poses from ck_rig_solve_host with those mounts.  Returns a dict."""
    from chalkydri_amd import rigcal as K
    from chalkydri_amd.rig import RigSolver
    rng = np.random.default_rng([seed, n_cams, n_steps])
    mounts = N.make_mounts(rng, n_cams)
    steps, truth, gyro = N.make_capture(rng, mounts, n_steps, noise=noise)
    start = N.perturb_mounts(rng, mounts)
    cs, m0 = c_steps(steps), [mount_iso(m) for m in start]
    solver = RigSolver()
    solver.params.sign_change_error = 0.0
    rr = solver.solve_host([[(t, b, m) for (t, b), m in zip(cams, m0)] for cams in cs], gyro)
    ok = [s for s in range(n_steps) if rr[s]["valid"]]
    return {"mounts": mounts, "start": start, "steps": steps, "csteps": cs, "m0": m0, "poses0": np.nan_to_num(K.start_poses(rr)), "ok": ok,
            "truth": truth, "n_cams": n_cams}


def shape_case(seed, n_cams, n_steps, n_tags, noise=1e-3):
    """One shape case of tests/test_gpu_rigcal.py: a synthetic capture with n_tags(s, c) tags per view, the mounts of cameras 1.. off by
    up to 1 degree and 1 cm, the poses by up to 0.02 rad and 3 cm."""
    rng = np.random.default_rng([seed, n_cams, n_steps])
    steps, mounts, poses = N.synthetic_capture(rng, n_cams, n_steps, n_tags, noise)
    start = N.perturb_mounts(rng, mounts, np.radians(1.0), 0.01)
    return {"csteps": c_steps(steps), "m0": [mount_iso(m) for m in start], "poses0": pose12(N.perturb_poses(rng, poses)), "n_cams": n_cams,
            "n_steps": n_steps}
