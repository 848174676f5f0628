#!/usr/bin/env python3
"""Generates tests/golden/pose_twin_golden.json: what the rig solver's host twin (ck_rig_solve_host, ck_rig_solve_robust_host;
DESIGN.md §4k, §4n) returns for a few problems of tests/np_rig.py::make_rig.  The GPU tests compare k_rig and k_rig_robust with the
twin; this fixture pins the twin itself, so that a change which moves twin and kernel together shows.  The inputs are stored, not
regenerated: numpy's sin / cos may differ in the last bit between machines.

Every array of every case lies in one byte string ("blob": base64 of its zlib stream; equal arrays once); a case names its arrays by
[offset, length].  A case is one step: "counts" tags per camera, the tags and bearings camera-major, one mount per camera, the heading.

    python tests/golden/make_pose_twin_golden.py        (rewrites the JSON; commit the result)
"""
import base64
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from make_cal_golden import Blob, isos  # noqa: E402

DBL_MAX = float(np.finfo(np.float64).max)


def to_step(cams):
    import np_rig as N
    from chalkydri_amd.sqpnp import iso3
    return [([iso3(t, N.mat_to_quat(R)) for R, t in tags], b, iso3(bb, N.mat_to_quat(Am))) for tags, b, (Am, bb) in cams]


def store(blob, name, step, gyro, rec, **more):
    case = {"name": name, "counts": [len(tags) for tags, _, _ in step],
            "tags": blob.put(isos(t for tags, _, _ in step for t in tags)),
            "bearings": blob.put(np.concatenate([np.asarray(b, np.float64).reshape(-1, 3) for _, b, _ in step])),
            "mounts": blob.put(isos(m for _, _, m in step)), "gyro": blob.put(np.array([gyro], np.float64)),
            "result": blob.put(rec.tobytes())}
    case.update(more)
    return case


def plain_cases(blob):
    import np_rig as N
    from chalkydri_amd.rig import RigSolver
    s, rng, out = RigSolver(), np.random.default_rng(20261020), []

    def add(name, step, gyro, check):
        rec = s.solve_host([step], [gyro])[0]
        assert check(rec), (name, rec)
        print("plain", name, "valid", int(rec["valid"]), "tags", list(rec["cam_tags"][:len(step)]), "energy", float(rec["energy"]))
        out.append(store(blob, name, step, gyro, rec))

    for n_cams in (1, 2, 3, 4, 8):
        for noise in (0.0, 1e-3):
            cams, gyro, _ = N.make_rig(rng, n_cams=n_cams, noise=noise, gyro_noise=0.02 if noise else 0.0)
            add("cams%d-%s" % (n_cams, "noise" if noise else "exact"), to_step(cams), gyro, lambda r: r["valid"] == 1)
    cams, gyro, _ = N.make_rig(rng, n_cams=2, noise=1e-3, tags_per_cam=(3, 3))
    step = to_step(cams)
    add("three-beside-none", [step[0], ([], np.zeros((0, 3)), step[1][2])], gyro,
        lambda r: r["valid"] == 1 and list(r["cam_tags"][:2]) == [3, 0])
    add("no-tag", [([], np.zeros((0, 3)), m) for _, _, m in step], gyro, lambda r: r.tobytes() == bytes(r.nbytes))
    cams, gyro, _ = N.make_rig(rng, n_cams=1, noise=1e-3, tags_per_cam=(1, 1))
    add("one-tag", to_step(cams), gyro, lambda r: r["valid"] == 1 and r["n_tags"] == 1)
    for attempt in range(20):                                            # bearing noise of 0.1: point-to-ray distances of 0.1-0.5 m
        cams, gyro, _ = N.make_rig(rng, n_cams=2, noise=0.1, tags_per_cam=(2, 3))
        step = to_step(cams)
        rec = s.solve_host([step], [gyro])[0]
        if rec["valid"] == 1 and rec["std_devs"][0] == DBL_MAX:
            break
    add("untrusted-rms", step, gyro, lambda r: r["valid"] == 1 and all(v == DBL_MAX for v in r["std_devs"]))
    return out


def robust_cases(blob):
    import np_rig_robust as NR
    from chalkydri_amd import _abi as A
    from chalkydri_amd.rig import RigSolver, RobustParams
    s, rng, out = RigSolver(), np.random.default_rng(20261021), []

    def add(name, case, max_rounds, check):
        step = to_step(case["cams"])
        rec = s.solve_host([step], [case["gyro"]], robust=RobustParams(max_rounds=max_rounds))[0]
        assert check(rec), (name, rec)
        print("robust", name, "status", int(rec["status"]), "rounds", int(rec["rounds"]), "rejected", int(rec["n_rejected"]))
        out.append(store(blob, name, step, case["gyro"], rec, max_rounds=max_rounds, planted=case["planted"]))
        return rec

    add("clean", NR.make_case(rng, 3, (2, 3), []), NR.MAX_ROUNDS,
        lambda r: (r["status"], r["rounds"], r["n_rejected"]) == (A.CK_RIG_ROBUST_CLEAN, 0, 0))
    wrong = NR.make_case(rng, 3, (3, 3), [(1, 2, "id")])               # one wrong tag in nine: within what GNC-TLS recovers
    full = add("wrong-tag", wrong, NR.MAX_ROUNDS,
               lambda r: r["status"] == A.CK_RIG_ROBUST_REJECTED and [int(m) for m in r["rejected"][:3]] == wrong["planted"])
    rounds = int(full["rounds"]) - 1
    assert rounds >= 2
    add("out-of-rounds", wrong, rounds, lambda r: r["status"] == A.CK_RIG_ROBUST_MAXROUNDS and r["rounds"] == rounds)
    return out


def main():
    blob = Blob()
    out = {"plain": plain_cases(blob), "robust": robust_cases(blob)}
    out["blob"] = base64.b64encode(zlib.compress(bytes(blob.data), 9)).decode()
    path = os.path.join(HERE, "pose_twin_golden.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    print(len(blob.data), "bytes of arrays,", os.path.getsize(path), "bytes of JSON")


if __name__ == "__main__":
    main()
