"""Per-tag pose without a GPU: the new C ABI symbols, defaults and layouts, the numpy restatement of the contract
(tests/np_tag_pose.py) against exact and rendered truth, the distortion path, and k_tagpose's register / scratch budget."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import np_tag_pose as T
import tag_pose_util as U
from chalkydri_amd import _abi as A
from chalkydri_amd import _lib, default_config, scenes, synth
from chalkydri_amd.detector import tag_pose_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = (900.0, 880.0, 640.0, 400.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def test_exports_and_defaults(built):
    L = _lib.lib()
    for name in ("ck_tag_pose_params_default", "ck_estimate_tag_poses", "ck_last_tag_poses"):
        assert hasattr(L, name), name
    pp = A.TagPoseParams()
    C.memset(C.byref(pp), 0xFF, C.sizeof(pp))
    L.ck_tag_pose_params_default(C.byref(pp))
    assert pp.n_iters == 50 and pp.pad == 0 and list(pp.tagsize) == [0.1651] * 4
    assert all(getattr(pp.cam, k) == 0.0 for k, _ in A.OpenCV5._fields_)
    assert L.ck_abi_version() == 3
    # without a handle every entry point refuses (no device is touched)
    out = (A.TagPose * 1)()
    assert L.ck_estimate_tag_poses(None, C.byref(pp), (A.Detection * 1)(), 1, out) == A.CK_EINVAL
    assert L.ck_last_tag_poses(None, C.byref(pp), out, 1, (C.c_int32 * 1)()) == A.CK_EINVAL
    q = tag_pose_params(500, 510, 320, 240, tagsize=[0.1, 0.2], distortion=(0.1, 0.01, 0.001, 0.002, 0.003), n_iters=7)
    assert (q.cam.fx, q.cam.fy, q.cam.cx, q.cam.cy, q.cam.k1, q.cam.k3, q.n_iters) == (500, 510, 320, 240, 0.1, 0.003, 7)
    assert list(q.tagsize) == [0.1, 0.2, 0.1651, 0.1651]


def test_ctypes_layout_matches_the_header():
    """sizeof / offsetof of both structs from a gcc-compiled probe of include/chalkydri_hip.h against the ctypes mirror."""
    fields = {"ck_tag_pose_params_t": ("cam", "tagsize", "n_iters", "pad"),
              "ck_tag_pose_t": ("id", "family", "valid", "has_alt", "R", "t", "err", "R_alt", "t_alt", "err_alt", "H")}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "chalkydri_hip.h"', "int main(void) {"]
    for st, fs in fields.items():
        src.append(f'printf("{st} size %zu\\n", sizeof({st}));')
        src += [f'printf("{st} {f} %zu\\n", offsetof({st}, {f}));' for f in fs]
    src.append("return 0; }")
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "probe.c"), os.path.join(td, "probe")
        open(c, "w").write("\n".join(src))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        lines = subprocess.check_output([exe], text=True).split("\n")
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in lines if ln}
    for st, cls in (("ck_tag_pose_params_t", A.TagPoseParams), ("ck_tag_pose_t", A.TagPose)):
        assert got[(st, "size")] == C.sizeof(cls)
        for f in fields[st]:
            assert got[(st, f)] == getattr(cls, f).offset, (st, f)
    assert C.sizeof(A.TagPoseParams) % 8 == 0 and C.sizeof(A.TagPose) % 8 == 0


def test_quartic_closed_form():
    """E(tau) = (a0 + ... + a4 tau^4) / (1 + tau^2)^2 equals E computed on R(tau) with the optimal translation."""
    rng = np.random.default_rng(3)
    s = 0.1651 / 2
    p = T.object_points(s)
    for _ in range(20):
        R, t = U.random_pose(rng)
        c = U.project(R, t, s, CAM) + rng.normal(0, 0.3, (4, 2))
        x, y, _ = T.undistort(CAM, c[:, 0], c[:, 1])
        v = np.stack([x, y, np.ones(4)], 1)
        F = T.calc_F(v)
        Minv = np.linalg.inv(np.eye(3) - F.mean(0))
        (a0, a1, a2, a3, a4), Rt, Rz, Rg, beta0 = T.quartic_coeffs(p, v, R, t)
        for tau in np.concatenate([np.linspace(-5, 5, 45), [-100.0, -0.01, 0.0, 0.01, 100.0]]):
            Rtau = T.R_of_tau(Rt, Rz, Rg, tau)
            topt = Minv @ ((np.einsum("kij,kj->ki", F, p @ Rtau.T) - p @ Rtau.T).sum(0) * 0.25)
            direct = T.object_error(p, v, Rtau, topt)
            closed = (a0 + tau * (a1 + tau * (a2 + tau * (a3 + tau * a4)))) / (1 + tau * tau) ** 2
            assert abs(closed - direct) <= 1e-10 * max(direct, 1e-300) + 1e-22, (tau, closed, direct)
        # R(beta0) is the rotation the family was built through
        assert np.abs(T.R_of_tau(Rt, Rz, Rg, math.tan(beta0 / 2)) - R).max() < 1e-12


def test_root_finder():
    for roots in ([-3.0, 0.5, 2.0, 7.0], [1.0, 1.0, -2.0, 4.0], [-999.0, -1.5, 0.25, 640.0]):
        P = np.poly(roots)[::-1] * 3.7                    # ascending coefficients
        got = T.poly_roots(list(P))
        want = sorted(set(roots))
        assert len(got) >= len(want) - 0 and all(min(abs(g - w) for g in got) < 1e-6 for w in want), (got, roots)
    assert T.poly_roots([1.0, 0.0, 0.0, 0.0, 0.0]) == []          # constant: no root
    assert all(np.isfinite(T.poly_roots([0.0, 0.0, 0.0, 0.0, 0.0])))  # zero polynomial: no NaN (zero there is no minimum)
    assert T.poly_roots([-2.0, 1.0, 0.0, 0.0, 0.0]) == [2.0]      # vanishing leading coefficients
    assert T.poly_roots([2000.0, 1.0]) == []                      # outside the search range


def _exact(n, seed, n_iters=1000):
    rng = np.random.default_rng(seed)
    s = 0.1651 / 2
    poses = [U.random_pose(rng) for _ in range(n)]
    corners = np.array([U.project(R, t, s, CAM) for R, t in poses])
    return poses, T.estimate_tag_poses(corners, [0] * n, list(range(n)), CAM, [0.1651], n_iters)


def test_exact_corners_recover_the_truth():
    poses, out = _exact(150, 4)
    hits = 0
    for (R, t), r in zip(poses, out):
        assert r["valid"]
        sols = [(r["R"], r["t"])] + ([(r["R_alt"], r["t_alt"])] if r["has_alt"] else [])
        errs = [max(np.abs(a - R).max(), np.abs(b - t).max() / np.linalg.norm(t)) for a, b in sols]
        assert min(errs) < 1e-6                                  # the truth is always one of {pose, alt}
        separated = not r["has_alt"] or U.rot_deg(r["R"], r["R_alt"]) > 5.0
        if separated:
            assert min(errs) < 1e-9
            hits += 1
    assert hits > 100


def test_both_minima_are_stationary():
    """Finite-difference gradient of E (optimal translation) over small rotations about both returned rotations is ~0."""
    poses, out = _exact(30, 5)
    s = 0.1651 / 2
    p = T.object_points(s)
    for (R, t), r in zip(poses, out):
        corners = U.project(R, t, s, CAM)
        x, y, _ = T.undistort(CAM, corners[:, 0], corners[:, 1])
        v = np.stack([x, y, np.ones(4)], 1)
        F = T.calc_F(v)
        Minv = np.linalg.inv(np.eye(3) - F.mean(0))

        def E(Rx):
            topt = Minv @ ((np.einsum("kij,kj->ki", F, p @ Rx.T) - p @ Rx.T).sum(0) * 0.25)
            return T.object_error(p, v, Rx, topt)
        for Rs in [r["R"]] + ([r["R_alt"]] if r["has_alt"] else []):
            h = 1e-5
            g = [(E(Rs @ U.rot(ax, h)) - E(Rs @ U.rot(ax, -h))) / (2 * h) for ax in np.eye(3)]
            curv = abs(E(Rs @ U.rot([1, 1, 0], 1e-2)) - E(Rs)) / 1e-4 + 1e-30
            assert max(abs(x) for x in g) <= 1e-5 * curv, (g, curv)


def test_rendered_frames_against_truth(oracle):
    rows = []
    for fam, dec, w, h in (("tag36h11", 2, 640, 480), ("tag16h5", 1, 320, 240)):
        cfg = default_config(w, h, families=(fam,), quad_decimate=dec)
        for seed in range(6):
            frame, truth = synth.render(1000 + seed, w, h, 6, families=(fam,))
            dets, _ = oracle.detect(frame, cfg)
            if not dets:
                continue
            out = T.estimate_tag_poses(np.array([d["p"] for d in dets]), [d["family"] for d in dets], [d["id"] for d in dets],
                                       (w, w, w / 2, h / 2, 0, 0, 0, 0, 0), [0.1651])
            for d, r in zip(dets, out):
                m = U.match_synth(d["p"], d["id"], truth)
                if m is not None:
                    rows.append(U.truth_errors(r, *U.synth_truth(m["H"], w, h, 0.1651)))
    e = np.array(rows)
    assert len(e) > 40
    assert np.median(e[:, 0]) <= U.TRUTH_ROT_MEDIAN_DEG and np.percentile(e[:, 0], 90) <= U.TRUTH_ROT_P90_DEG
    assert e[:, 1].max() <= U.TRUTH_ROT_BEST_DEG and e[:, 2].max() <= U.TRUTH_T_REL
    w, h, f = 1280, 800, 800.0
    layout = scenes.wall_layout(6)
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
    cfg = default_config(w, h)
    rows = []
    for i, pose in enumerate([(1.0, 0.2, 0.1), (2.5, -0.4, -0.2), (3.2, 0.5, 0.25)]):
        frame, _ = scenes.render_view(90 + i, w, h, f, layout, pose, r2c)
        truth = U.view_truths(layout, pose, r2c)
        dets, _ = oracle.detect(frame, cfg)
        out = T.estimate_tag_poses(np.array([d["p"] for d in dets]).reshape(-1, 4, 2), [0] * len(dets), [d["id"] for d in dets],
                                   (f, f, w / 2, h / 2, 0, 0, 0, 0, 0), [0.1651])
        rows += [U.truth_errors(r, *truth[d["id"]]) for d, r in zip(dets, out)]
    e = np.array(rows)
    assert len(e) >= 10 and e[:, 1].max() <= U.TRUTH_ROT_BEST_DEG and e[:, 2].max() <= U.TRUTH_T_REL


def test_distortion_path_gives_the_pinhole_pose():
    """Corners distorted with the OpenCV-5 forward model, undistorted by the contract's iteration, give the pinhole pose."""
    cam = (1368.33, 1368.51, 784.10, 655.20, -0.0343, -0.00212, -0.001, -0.000141, 0.0153)   # scenes.REF_CALIB
    pin = cam[:4] + (0.0,) * 5
    rng = np.random.default_rng(6)
    s = 0.1651 / 2
    poses = [U.random_pose(rng, 0.5, 6.0) for _ in range(40)]
    undist = np.array([U.project(R, t, s, pin) for R, t in poses])
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    x, y = (undist[..., 0] - cx) / fx, (undist[..., 1] - cy) / fy
    r2 = x * x + y * y
    radial = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    dist = np.stack([xd * fx + cx, yd * fy + cy], -1)
    a = T.estimate_tag_poses(dist, [0] * 40, list(range(40)), cam, [0.1651])
    b = T.estimate_tag_poses(undist, [0] * 40, list(range(40)), pin, [0.1651])
    for ra, rb in zip(a, b):
        assert ra["valid"] and rb["valid"] and ra["has_alt"] == rb["has_alt"]
        assert np.abs(ra["R"] - rb["R"]).max() < 1e-7 and np.abs(ra["t"] - rb["t"]).max() < 1e-7 * max(1, np.linalg.norm(rb["t"]))
    # zero distortion: the iteration returns the pinhole formula bit for bit
    u = rng.uniform(0, 1280, 64)
    v = rng.uniform(0, 800, 64)
    x, y, ok = T.undistort(pin, u, v)
    assert ok.all() and np.array_equal(x, (u - pin[2]) / pin[0]) and np.array_equal(y, (v - pin[3]) / pin[1])


def test_degenerate_corners_in_the_restatement():
    good = U.project(U.rot([1, 0.2, 0], 0.3), np.array([0.1, 0.0, 2.0]), 0.08, CAM)
    cases = [np.full((4, 2), 50.0), np.array([[1.0, 1], [2, 2], [3, 3], [4, 4]]), np.where(np.arange(8).reshape(4, 2) == 5, np.nan, good)]
    out = T.estimate_tag_poses(np.array(cases), [0, 0, 0], [1, 2, 3], CAM, [0.1651])
    assert [r["valid"] for r in out] == [0, 0, 0]
    out = T.estimate_tag_poses(good[None], [3], [9], CAM, [0.1651])      # family outside the handle's one
    assert out[0]["valid"] == 0 and out[0]["family"] == 3


def _notes(obj):
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    res = {}
    with tempfile.TemporaryDirectory() as td:
        import shutil
        shutil.copy(obj, td)
        name = os.path.basename(obj)
        subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", name], cwd=td, stdout=subprocess.DEVNULL)
        co = [f for f in os.listdir(td) if f.startswith(name) and "amdgcn" in f][0]
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], cwd=td, text=True)
    kname = None
    for line in notes.splitlines():
        m = re.match(r"\s*\.name:\s+(\S+)", line)
        if m:
            kname = m.group(1)
            res[kname] = {}
        m = re.match(r"\s*\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)", line)
        if m and kname:
            res[kname][m.group(1)] = int(m.group(2))
    return res


def test_tagpose_kernel_keeps_its_budget(built):
    """k_tagpose: no spill and no more scratch than k_sqpnp's 32 bytes (it has none); k_sqpnp keeps its own figure after the
    3x3 helpers moved to a header of their own (ck_pose_math.h)."""
    build = os.path.join(ROOT, "chalkydri_amd", "csrc", "build")
    tp = [v for k, v in _notes(os.path.join(build, "k_tagpose.o")).items() if "k_tagpose" in k]
    sq = [v for k, v in _notes(os.path.join(build, "k_sqpnp.o")).items() if "7k_sqpnp" in k]
    assert tp and sq
    for v in tp:
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] <= 32, v
    for v in sq:
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] <= 32, v


if __name__ == "__main__":
    sys.exit(pytest.main([__file__, "-q"]))
