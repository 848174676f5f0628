#!/usr/bin/env python3
"""Generates tests/golden/cal_twin_golden.json: what the three calibration twins (ck_calib_refine_host, ck_rigcal_refine_host,
ck_fieldcal_refine_host) return, byte for byte, for a few of the shape cases of the GPU tests.  The GPU tests
compare the kernels with the twins; this fixture pins the twins themselves, so that a change which moves twin and kernel together
shows.  The inputs are stored, not regenerated: numpy's sin / cos may differ in the last bit between machines.

Every array of every case lies in one byte string ("blob": base64 of its zlib stream; equal arrays once); a case names its arrays by
[offset, length].  The cases are built with the helpers and seeds of tests/test_gpu_*.py; cams8 with one tag per view.

    python tests/golden/make_cal_golden.py        (rewrites the JSON; commit the result)
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

RIGCAL = ("absent", "cams8", "skipped", "position_frozen", "maxit")
FIELDCAL = ("tags3", "cams2_cams3", "absent", "unseen", "masks", "maxit")
CALIB = (("F3", 0, 100), ("F4", "FIX_DISTORTION", 100), ("F4", 0, 3))


class Blob:
    def __init__(self):
        self.data, self.seen = bytearray(), {}

    def put(self, a):
        b = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
        if b not in self.seen:
            self.seen[b] = [len(self.data), len(b)]
            self.data += b
        return self.seen[b]


def isos(seq):
    return b"".join(bytes(t) for t in seq)


def rigcal_cases(blob):
    import rigcal_cases as RC
    import test_gpu_rigcal as T
    from chalkydri_amd import rigcal as K
    out = []
    for name in RIGCAL:
        n_cams, n_steps, n_tags, mask, max_iters, min_steps = T.CASES[name]
        if name == "cams8":
            n_tags = lambda s, c: 1
        case = RC.shape_case(3, n_cams, n_steps, n_tags)
        p = K.params(mask, max_iters=max_iters, min_steps=min_steps)
        res, poses = K.refine_host(p, K.Capture(case["csteps"]), case["m0"], case["poses0"])
        print("rigcal", name, "status", int(res["status"]), "iters", int(res["iters"]), "used", int(res["n_steps_used"]))
        out.append({"name": name, "n_cams": n_cams, "fixed_mask": mask, "max_iters": max_iters, "min_steps": min_steps,
                    "counts": [[len(tg) for tg, _ in cams] for cams in case["csteps"]],
                    "tags": blob.put(isos(t for cams in case["csteps"] for tg, _ in cams for t in tg)),
                    "bearings": blob.put(np.concatenate([b.reshape(-1, 3) for cams in case["csteps"] for _, b in cams])),
                    "mounts0": blob.put(isos(case["m0"])), "poses0": blob.put(case["poses0"]),
                    "result": blob.put(res.tobytes()), "poses": blob.put(poses)})
    return out


def fieldcal_cases(blob):
    import fieldcal_cases as FC
    import test_gpu_fieldcal as T
    from chalkydri_amd import fieldcal as K
    out = []
    for name in FIELDCAL:
        n_cams, n_steps, n_layout, seen, masks, max_iters, min_steps = T.CASES[name]
        case = FC.shape_case(3, n_cams, n_steps, n_layout, seen, masks=masks)
        p = K.params(max_iters=max_iters, min_steps=min_steps)
        res, lay, sight, rms, poses = K.refine_host(p, K.Capture(case["steps"]), case["m_iso"], case["lay0"], case["fixed"], case["poses0"])
        print("fieldcal", name, "status", int(res["status"]), "iters", int(res["iters"]), "used", int(res["n_steps_used"]))
        out.append({"name": name, "n_cams": n_cams, "max_iters": max_iters, "min_steps": min_steps,
                    "ids": [[[int(k) for k in ids] for ids, _ in cams] for cams in case["steps"]],
                    "bearings": blob.put(np.concatenate([np.asarray(b, np.float64).reshape(-1, 3) for cams in case["steps"] for _, b in cams])),
                    "mounts": blob.put(isos(case["m_iso"])), "layout0": blob.put(isos(case["lay0"])), "fixed": blob.put(case["fixed"]),
                    "poses0": blob.put(case["poses0"]), "result": blob.put(res.tobytes()), "layout": blob.put(lay), "sightings": blob.put(sight),
                    "tag_rms": blob.put(rms), "poses": blob.put(poses)})
    return out


def calib_cases(blob):
    import test_gpu_calib as T
    from chalkydri_amd import _abi as A
    from chalkydri_amd import calibration as K
    out = []
    for shape, mask, iters in CALIB:
        m = A.CK_CALIB_FIX_DISTORTION if mask == "FIX_DISTORTION" else mask
        frames = T._frames(T.SHAPES[shape], 40 + sorted(T.SHAPES).index(shape))
        p = K.params(T.W, T.H, fixed_mask=m, max_iters=iters)
        cam0, poses0, st = K.calib_init(p, frames)
        assert st == A.CK_CALIB_CONVERGED
        res, poses = K.refine_host(p, frames, cam0, poses0)
        print("calib", shape, mask, iters, "status", int(res["status"]), "iters", int(res["iters"]))
        out.append({"name": "%s-mask%x-it%d" % (shape, m, iters), "width": T.W, "height": T.H, "fixed_mask": m, "max_iters": iters,
                    "counts": [len(b) for b, _ in frames], "board_xy": blob.put(np.concatenate([b for b, _ in frames])),
                    "image_uv": blob.put(np.concatenate([u for _, u in frames])), "cam0": blob.put(cam0), "poses0": blob.put(poses0),
                    "result": blob.put(res.tobytes()), "poses": blob.put(poses)})
    return out


def main():
    blob = Blob()
    out = {"rigcal": rigcal_cases(blob), "fieldcal": fieldcal_cases(blob), "calib": calib_cases(blob)}
    out["blob"] = base64.b64encode(zlib.compress(bytes(blob.data), 9)).decode()
    path = os.path.join(HERE, "cal_twin_golden.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    print(len(blob.data), "bytes of arrays,", os.path.getsize(path), "bytes of JSON")


if __name__ == "__main__":
    main()
