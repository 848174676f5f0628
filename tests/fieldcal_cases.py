"""What the field calibration tests share: the conversion of np_fieldcal's scenes to the C ABI's records, the
acceptance captures of the CPU tests and the small shape cases of the GPU tests."""
import ctypes as C
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_fieldcal as N  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

FIX_ALL = 63


def iso(R, t):
    return A.Iso3((C.c_double * 3)(*t), (C.c_double * 4)(*N.mat_to_quat(R)))


def mount_iso(m):
    """(A, o) -> robot_to_cam (A, b = -A o)"""
    return iso(m[0], -m[0] @ m[1])


def layout_of(recs):
    """layout records of a result -> [(Q, c)]"""
    return [(N.quat_to_mat(r["q"]), np.array(r["t"], float)) for r in recs]


def pose12(poses):
    return np.array([np.concatenate([R.reshape(9), t]) for R, t in poses]).reshape(-1, 12)


def fixed_of(n_layout, masks):
    fx = np.zeros(n_layout, np.uint8)
    for k, m in masks.items():
        fx[k] = m
    return fx


def field_json_layout(path=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field.json")):
    """(ids, [(Q, c)], field size) of a field.json"""
    import json
    d = json.load(open(path))
    q = lambda t: [t["pose"]["rotation"]["quaternion"][a] for a in "WXYZ"]
    return ([t["ID"] for t in d["tags"]], [(N.quat_to_mat(q(t)), np.array([t["pose"]["translation"][a] for a in "xyz"])) for t in d["tags"]],
            (d["field"]["length"], d["field"]["width"]))


@functools.lru_cache(maxsize=None)
def acceptance_case(n_cams, n_steps, seed, noise, field=False):
    """One acceptance input of tests/test_fieldcal_host.py: the room of np_rigcal (8 x 6 m, 28 wall tags); the true layout is the
    nominal one with every tag but the gauge (the tag with the most sightings) moved by up to 3 cm and 2 degrees; the starts are the
    nominal layout and the poses of ck_rig_solve_host with it.  Returns a dict; `ok` = the steps that solver has a pose for."""
    from chalkydri_amd import rigcal as K
    from chalkydri_amd.rig import RigSolver
    rng = np.random.default_rng([seed, n_cams, n_steps, 4])
    nominal, size = (N.room_tags(), (8.0, 6.0)) if not field else field_json_layout()[1:]   # (field=True: the 32 tags of tests/golden/field.json)
    mounts = N.make_mounts(rng, n_cams)
    true = N.perturb_layout(rng, nominal, keep=())
    steps, truth, gyro = N.make_capture(rng, mounts, true, n_steps, noise=noise, width=size[0], depth=size[1])
    count = np.bincount([k for cams in steps for ids, _ in cams for k in ids], minlength=len(nominal))
    gauge = int(np.argmax(count))
    nominal[gauge] = true[gauge]                                             # the gauge tag is where the drawing says
    lay0, m_iso = [iso(Q, c) for Q, c in nominal], [mount_iso(m) for m in mounts]
    solver = RigSolver()
    solver.params.sign_change_error = 0.0
    rr = solver.solve_host([[([lay0[k] for k in ids], b, m) for (ids, b), m in zip(cams, m_iso)] for cams in steps], gyro)
    ok = [s for s in range(n_steps) if rr[s]["valid"]]
    return {"nominal": nominal, "true": true, "mounts": mounts, "m_iso": m_iso, "lay0": lay0, "steps": steps, "gauge": gauge,
            "fixed": fixed_of(len(nominal), {gauge: FIX_ALL}), "poses0": np.nan_to_num(K.start_poses(rr)), "ok": ok, "truth": truth,
            "gyro": gyro, "n_cams": n_cams, "n_steps": n_steps}


def shape_case(seed, n_cams, n_steps, n_layout, seen, noise=1e-3, masks=None):
    """One shape case of tests/test_gpu_fieldcal.py: a synthetic capture in which camera c at step s has the tags seen(s, c), tag 0
    the gauge (or `masks`: {entry: mask}), the other tags of the start layout off by up to 1 degree and 1 cm, the poses by up to
    0.02 rad and 3 cm."""
    rng = np.random.default_rng([seed, n_cams, n_steps, n_layout])
    steps, mounts, layout, poses = N.synthetic_capture(rng, n_cams, n_steps, n_layout, seen, noise)
    masks = {0: FIX_ALL} if masks is None else masks
    start = N.perturb_layout(rng, layout, np.radians(1.0), 0.01, keep=[k for k, m in masks.items() if m == FIX_ALL])
    return {"steps": steps, "m_iso": [mount_iso(m) for m in mounts], "lay0": [iso(Q, c) for Q, c in start], "fixed": fixed_of(n_layout, masks),
            "poses0": pose12(N.perturb_poses(rng, poses)), "n_cams": n_cams, "n_steps": n_steps, "layout": layout, "poses": poses}


def ring(n_tags, per_step, stride=1):
    """seen(s, c) of a capture that walks a ring of n_tags tags: every camera sees per_step consecutive tags from (s * stride + c)"""
    return lambda s, c: [(s * stride + c + j) % n_tags for j in range(per_step)]
