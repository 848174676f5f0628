"""The three calibration twins (ck_calib_refine_host, ck_rigcal_refine_host, ck_fieldcal_refine_host) against
the bytes they returned when tests/golden/cal_twin_golden.json was written (tests/golden/make_cal_golden.py).  The GPU tests compare
each kernel with its twin, so a change that moves both together passes them; this test holds the twins where they were.  The fixture
stores the inputs themselves; the twins use only + - * / sqrt with -ffp-contract=off, so the bytes do not depend on the compiler."""
import base64
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

from chalkydri_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "cal_twin_golden.json")))
BLOB = zlib.decompress(base64.b64decode(GOLDEN["blob"]))


def raw(at):
    return BLOB[at[0]:at[0] + at[1]]


def f64(at, *shape):
    return np.frombuffer(raw(at), np.float64).reshape(*shape).copy()


def isos(at):
    b = raw(at)
    return [A.Iso3.from_buffer_copy(b[i:i + C.sizeof(A.Iso3)]) for i in range(0, len(b), C.sizeof(A.Iso3))]


@pytest.mark.parametrize("g", GOLDEN["rigcal"], ids=[g["name"] for g in GOLDEN["rigcal"]])
def test_rigcal_twin(built, g):
    from chalkydri_amd import rigcal as K
    tags, bear, at = isos(g["tags"]), f64(g["bearings"], -1, 3), 0
    steps = []
    for counts in g["counts"]:
        cams = []
        for n in counts:
            cams.append((tags[at:at + n], bear[4 * at:4 * (at + n)]))
            at += n
        steps.append(cams)
    p = K.params(g["fixed_mask"], max_iters=g["max_iters"], min_steps=g["min_steps"])
    res, poses = K.refine_host(p, K.Capture(steps), isos(g["mounts0"]), f64(g["poses0"], -1, 12))
    assert res.tobytes() == raw(g["result"]), (g["name"], res)
    assert poses.tobytes() == raw(g["poses"]), g["name"]


@pytest.mark.parametrize("g", GOLDEN["fieldcal"], ids=[g["name"] for g in GOLDEN["fieldcal"]])
def test_fieldcal_twin(built, g):
    from chalkydri_amd import fieldcal as K
    bear, at = f64(g["bearings"], -1, 3), 0
    steps = []
    for per_cam in g["ids"]:
        cams = []
        for ids in per_cam:
            cams.append((ids, bear[at:at + 4 * len(ids)]))
            at += 4 * len(ids)
        steps.append(cams)
    p = K.params(max_iters=g["max_iters"], min_steps=g["min_steps"])
    got = K.refine_host(p, K.Capture(steps), isos(g["mounts"]), isos(g["layout0"]), np.frombuffer(raw(g["fixed"]), np.uint8), f64(g["poses0"], -1, 12))
    for what, a in zip(("result", "layout", "sightings", "tag_rms", "poses"), got):
        assert a.tobytes() == raw(g[what]), (g["name"], what, a)


@pytest.mark.parametrize("g", GOLDEN["calib"], ids=[g["name"] for g in GOLDEN["calib"]])
def test_calib_twin(built, g):
    from chalkydri_amd import calibration as K
    bxy, uv, at = f64(g["board_xy"], -1, 2), f64(g["image_uv"], -1, 2), 0
    frames = []
    for n in g["counts"]:
        frames.append((bxy[at:at + n], uv[at:at + n]))
        at += n
    p = K.params(g["width"], g["height"], fixed_mask=g["fixed_mask"], max_iters=g["max_iters"])
    res, poses = K.refine_host(p, frames, f64(g["cam0"], 9), f64(g["poses0"], -1, 12))
    assert res.tobytes() == raw(g["result"]), (g["name"], res)
    assert poses.tobytes() == raw(g["poses"]), g["name"]
