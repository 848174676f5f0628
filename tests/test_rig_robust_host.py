"""The robust rig solve on the host (ck_rig_solve_robust_host, chalkydri_amd/csrc/ck_rig_host.c) against its numpy
restatement (tests/np_rig_robust.py) on scenes with planted outliers, against the plain solve on clean scenes and on the scenes with
the planted tags deleted, its refusals, and the code object of the kernel that runs the same arithmetic.  No device is needed: the
device solver is compared with this twin in tests/test_gpu_rig_robust.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_rig as N  # noqa: E402
import np_rig_robust as NR  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd.rig import ROBUST_RESULT_DTYPE, RigSolver, RobustParams, pack_steps  # noqa: E402
from chalkydri_amd.sqpnp import iso3  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9          # tests/test_rig_host.py::test_twin_matches_restatement's bound on rot, pos, yaw, std_devs, cam_rms; relative on energy


def to_step(cams):
    return [([iso3(t, N.mat_to_quat(R)) for R, t in tags], b, iso3(bb, N.mat_to_quat(Am))) for tags, b, (Am, bb) in cams]


def masks(rec, n_cams):
    assert not rec["rejected"][n_cams:].any()
    return [int(m) for m in rec["rejected"][:n_cams]]


def close(got, want):
    """a fused record against np_rig's record"""
    assert got["valid"] == 1 and got["n_tags"] == want["n_tags"]
    assert list(got["cam_tags"][:len(want["cam_tags"])]) == want["cam_tags"]
    assert np.abs(got["rot"] - want["rot"]).max() < TOL and np.abs(got["pos"] - want["pos"]).max() < TOL
    assert abs(got["yaw"] - want["yaw"]) < TOL and np.abs(got["std_devs"] - want["std"]).max() < TOL
    assert np.abs(got["cam_rms"][:len(want["cam_rms"])] - want["cam_rms"]).max() < TOL
    assert abs(got["energy"] - want["energy"]) <= TOL * want["energy"] + 1e-12


@pytest.fixture(scope="module")
def cases():
    return NR.suite()


@pytest.fixture(scope="module")
def restated(cases):
    """the restatement of every case, once"""
    return {k: [NR.solve_robust(c["cams"], c["gyro"]) for c in v] for k, v in cases.items()}


@pytest.fixture(scope="module")
def twin(built, cases):
    s = RigSolver()
    return {k: s.solve_host([to_step(c["cams"]) for c in v], [c["gyro"] for c in v], robust=True) for k, v in cases.items()}


def test_restatement_recovers_the_planted_tags(cases, restated):
    """The condition the other tests stand on, with no case left out: GNC-TLS, as restated in numpy, rejects exactly the planted tags
    of every generated case (and nothing of a clean one)."""
    n = n_out = 0
    for k, v in cases.items():
        for c, r in zip(v, restated[k]):
            assert r["rejected"] == c["planted"], (k, c["planted"], r["rejected"])
            assert r["status"] == (NR.REJECTED if any(c["planted"]) else NR.CLEAN) and (r["rounds"] > 0) == any(c["planted"])
            n += 1
            n_out += any(c["planted"])
    print(n, "cases,", n_out, "with outliers")
    assert n >= 40 and n_out >= 25


def test_twin_matches_restatement(cases, restated, twin):
    for k, v in cases.items():
        for c, want, got in zip(v, restated[k], twin[k]):
            assert (got["status"], got["rounds"], got["n_rejected"]) == (want["status"], want["rounds"], int((~want["keep"]).sum()))
            assert masks(got, k) == want["rejected"]
            close(got["fused"], want["fused"])
            assert abs(got["worst_inlier_rad"] - want["worst"]) < TOL and abs(got["best_rejected_rad"] - want["best"]) < TOL
            if want["rounds"]:
                assert got["worst_inlier_rad"] <= NR.GATE < got["best_rejected_rad"]


def test_clean_input_is_the_plain_solve(cases, twin):
    """no outlier: `fused` is ck_rig_solve_host's record byte for byte, status CLEAN, no round"""
    s, n = RigSolver(), 0
    for k, v in cases.items():
        plain = s.solve_host([to_step(c["cams"]) for c in v], [c["gyro"] for c in v])
        for c, p, got in zip(v, plain, twin[k]):
            if any(c["planted"]):
                continue
            n += 1
            assert got["fused"].tobytes() == p.tobytes() and p["valid"]
            assert (got["status"], got["rounds"], got["n_rejected"]) == (A.CK_RIG_ROBUST_CLEAN, 0, 0) and masks(got, k) == [0] * k
            assert got["best_rejected_rad"] == 0.0 and 0.0 < got["worst_inlier_rad"] <= NR.GATE
    assert n >= 10


def test_robust_is_the_plain_solve_without_the_planted_tags(cases, twin):
    """... and with outliers `fused` is ck_rig_solve_host on the input with the planted tags deleted"""
    s, n = RigSolver(), 0
    for k, v in cases.items():
        gyro = [c["gyro"] for c in v]
        deleted = s.solve_host([to_step(NR.delete_planted(c)) for c in v], gyro)
        for c, d, got in zip(v, deleted, twin[k]):
            if not any(c["planted"]):
                continue
            n += 1
            f = got["fused"]
            assert np.abs(f["rot"] - d["rot"]).max() < TOL and np.abs(f["pos"] - d["pos"]).max() < TOL and abs(f["yaw"] - d["yaw"]) < TOL
            assert abs(f["energy"] - d["energy"]) <= TOL * d["energy"] and f["n_tags"] == d["n_tags"]
            assert np.array_equal(f["cam_tags"], d["cam_tags"])
    assert n >= 25


def test_empty_step_and_no_consensus(built, cases):
    s = RigSolver()
    c = cases[3][0]
    step = to_step(c["cams"])
    empty = [([], np.zeros((0, 3)), m) for _, _, m in step]
    res = s.solve_host([step, empty], [c["gyro"], 0.0], robust=True)
    assert res[0]["status"] == A.CK_RIG_ROBUST_REJECTED and res[1].tobytes() == bytes(res[1].nbytes)
    # more inliers asked for than survive: no pose, and the record says which tags fell
    n_in = int(res[0]["fused"]["n_tags"])
    r = s.solve_host([step], [c["gyro"]], robust=RobustParams(min_inlier_tags=n_in + 1))[0]
    assert r["status"] == A.CK_RIG_ROBUST_NO_CONSENSUS and r["fused"].tobytes() == bytes(r["fused"].nbytes)
    assert masks(r, 3) == c["planted"] and r["n_rejected"] == 1 and r["worst_inlier_rad"] == 0.0
    r = s.solve_host([step], [c["gyro"]], robust=RobustParams(min_inlier_tags=n_in))[0]
    assert r.tobytes() == res[0].tobytes()
    # ... also where no round ran
    clean = cases[1][0]
    r = s.solve_host([to_step(clean["cams"])], [clean["gyro"]], robust=RobustParams(min_inlier_tags=2))[0]
    assert r["status"] == A.CK_RIG_ROBUST_NO_CONSENSUS and r["fused"]["valid"] == 0
    # one round fewer than the weights need to settle: MAXROUNDS, the inliers by w >= 0.5, still a pose of them; a single round: every
    # weight is still far below 0.5 (mu starts small: the surrogate cost starts near the convex one), so nothing is left
    full = int(res[0]["rounds"])
    r = s.solve_host([step], [c["gyro"]], robust=RobustParams(max_rounds=full - 1))[0]
    assert full > 2 and r["status"] == A.CK_RIG_ROBUST_MAXROUNDS and r["rounds"] == full - 1
    assert r["fused"]["valid"] == 1 and r["fused"]["n_tags"] + r["n_rejected"] == n_in + 1
    r = s.solve_host([step], [c["gyro"]], robust=RobustParams(max_rounds=1))[0]
    assert r["status"] == A.CK_RIG_ROBUST_NO_CONSENSUS and r["rounds"] == 1 and r["n_rejected"] == n_in + 1


def misuse(call):
    """the refusals both stand-alone entry points share; call(params, n_cams, probs, n, tarr, nt, barr, gyro) -> rc"""
    rng = np.random.default_rng(5)
    cams, gyro, _ = N.make_rig(rng, n_cams=2, noise=1e-3, tags_per_cam=(2, 2))
    n_cams, probs, tarr, nt, barr = pack_steps([to_step(cams)])
    g = np.array([gyro])
    L = RigSolver()._L

    def prm(**kw):
        p = A.RigRobustParams()
        L.ck_rig_robust_params_default(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    d = prm()
    assert (d.gate_rad, d.mu_factor, d.max_rounds, d.min_inlier_tags, d.rig.rig_id, d.rig.sqpnp.max_iter) == (0.01, 1.4, 64, 1, 255, 15)
    assert call(d, n_cams, probs, 1, tarr, nt, barr, g) == A.CK_OK
    for kw in ({"gate_rad": 0.0}, {"gate_rad": -0.01}, {"gate_rad": float("nan")}, {"gate_rad": float("inf")}, {"mu_factor": 1.0},
               {"mu_factor": 0.5}, {"max_rounds": 0}, {"min_inlier_tags": 0}):
        assert call(prm(**kw), n_cams, probs, 1, tarr, nt, barr, g) == A.CK_EINVAL, kw
        assert call(prm(**kw), n_cams, probs, 0, tarr, nt, barr, g) == A.CK_EINVAL, kw
    assert call(d, 0, probs, 1, tarr, nt, barr, g) == A.CK_EINVAL and call(d, 9, probs, 1, tarr, nt, barr, g) == A.CK_EINVAL
    assert call(None, n_cams, probs, 1, tarr, nt, barr, g) == A.CK_EINVAL
    keep = probs[0].n_bearings
    probs[0].n_bearings = keep - 1                                                   # the plain call's checks come along
    assert call(d, n_cams, probs, 1, tarr, nt, barr, g) == A.CK_EINVAL
    probs[0].n_bearings = keep
    # 65 tags in one camera's record: more than a mask has bits
    tags, b, m = to_step(cams)[0]
    big = [((tags * 33)[:n], np.tile(b, (33, 1))[:4 * n], m) for n in (64, 65)]
    for view, want in zip(big, (A.CK_OK, A.CK_EINVAL)):
        n1, p1, t1, nt1, b1 = pack_steps([[view]])
        assert call(d, n1, p1, 1, t1, nt1, b1, g) == want


def test_misuse(built):
    L = RigSolver()._L

    def call(p, n_cams, probs, n, tarr, nt, barr, g):
        res = np.zeros(max(n, 1), ROBUST_RESULT_DTYPE)
        return L.ck_rig_solve_robust_host(None if p is None else C.byref(p), n_cams, probs, n, tarr, nt, barr.ctypes.data, len(barr),
                                          g.ctypes.data, res.ctypes.data_as(C.POINTER(A.RigRobustResult)))
    misuse(call)
    with pytest.raises(TypeError):
        RigSolver().solve_host([], [], robust=1.5)


def test_determinism(cases, twin):
    s = RigSolver()
    again = s.solve_host([to_step(c["cams"]) for c in cases[8]], [c["gyro"] for c in cases[8]], robust=True)
    assert again.tobytes() == twin[8].tobytes()


def test_robust_kernel_uses_no_private_segment(built):
    """k_rig_robust keeps its per-tag state in LDS and its per-lane arrays in registers: the gfx950 code object's metadata shows a
    private segment of 0 bytes and no spilled vector register (read as tests/test_abi.py reads the fit kernels' budgets); k_rig, whose
    body it shares, likewise."""
    import shutil
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    res = {}
    with tempfile.TemporaryDirectory() as td:
        obj = "k_rigpnp.o"
        shutil.copy(os.path.join(ROOT, "chalkydri_amd", "csrc", "build", obj), td)
        subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", obj], cwd=td, stdout=subprocess.DEVNULL)
        co = [f for f in os.listdir(td) if f.startswith(obj) and "amdgcn" in f][0]
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], cwd=td, text=True)
        name = None
        for line in notes.splitlines():
            m = re.match(r"\s*\.name:\s+(\S+)", line)
            if m:
                name = m.group(1)
                res[name] = {}
            m = re.match(r"\s*\.(vgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)", line)
            if m and name:
                res[name][m.group(1)] = int(m.group(2))
    robust = [v for k, v in res.items() if "k_rig_robust" in k]
    plain = [v for k, v in res.items() if "k_rig" in k and "k_rig_robust" not in k]
    print(res)
    assert len(robust) == 1 and len(plain) == 1
    for v in robust + plain:
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, v
