"""k_rig and k_rig_robust (chalkydri_amd/csrc/k_rigpnp.hip) record for record at their own edges: the cases of
tests/rig_cases.py (tests/test_rig_cases_host.py proves on the CPU that each reaches the edge it is named for), one solve_batch per
case on one 64 x 64 handle, against the host twin (integers and masks equal, continuous fields within 1e-9: what
tests/test_gpu_rig.py demands) and against the numpy restatement (discrete fields exact, continuous ones within the step's
max(1e-9, 64 kappa) of rig_cases.restated: the comparison that can see a wrong branch in the shared ck_pose_math.h).  Then the
identities that need no tolerance: empty cameras, planted tags, clean robust steps, the position in the batch, two runs."""
import numpy as np
import pytest

import np_rig_robust as NR
import rig_cases as rc

from chalkydri_amd import _abi as A
from chalkydri_amd._lib import ChalkydriError
from chalkydri_amd.rig import RigSolver

pytestmark = pytest.mark.gpu
ROBUST = tuple(n for n in rc.NAMES if n.startswith("count_") and n.endswith("_robust"))


@pytest.fixture(scope="module")
def det(built):
    from chalkydri_amd.detector import AprilTagDetector
    d = AprilTagDetector(64, 64)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev(det):
    return RigSolver(det)


@pytest.fixture(scope="module")
def solved(dev):
    """the device's records of a case: one solve_batch per case, once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = rc.solve(dev, rc.case(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", rc.NAMES)
def test_device_matches_twin(solved, name):
    """every step, the twin-only ones included"""
    c = rc.case(name)
    got, want = solved(name), rc.solve(RigSolver(), c, host=True)
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        worst = max(worst, rc.against_twin(f"{name}[{i}] device vs twin", c, g, w))
    print(name, "device vs twin: worst", worst)


@pytest.mark.parametrize("name", [n for n in rc.NAMES if not rc.case(n)["twin_only"]])
def test_device_matches_restatement(solved, name):
    c = rc.case(name)
    worst = 0.0
    for i, (g, s) in enumerate(zip(solved(name), rc.restated(name))):
        worst = max(worst, rc.against_restatement(f"{name}[{i}] device vs restatement", c, g, s))
    print(name, "device vs restatement: worst", worst, "bound", max(s["bound"] for s in rc.restated(name)))


def test_sparse_cameras_are_the_compacted_step(dev, solved):
    """empty cameras at the front, in a row, all but the last: the record of the step with the empty cameras deleted, byte for byte"""
    c = rc.case("cams_sparse")
    for i, (cams, g) in enumerate(zip(c["steps"], solved("cams_sparse"))):
        small, idx = rc.compact(cams)
        w = dev.solve_batch([rc.to_step(small)], [c["gyro"][i]])[0]
        assert g["valid"] == 1
        rc.same_but_for_the_cameras(f"cams_sparse[{i}] device", g, w, idx)


@pytest.mark.parametrize("name", ROBUST)
def test_planted_tags_are_deleted(dev, solved, name):
    """the masks are exactly the planted bits (bit 63 included) and `fused` is the plain solve of the input without the planted tags"""
    c = rc.case(name)
    got = solved(name)
    planted = [i for i, p in enumerate(c["planted"]) if any(p)]
    assert planted
    deleted = []
    for i in planted:
        keep = [not (c["planted"][i][k] >> t) & 1 for k, (tags, _, _) in enumerate(c["steps"][i]) for t in range(len(tags))]
        deleted.append(rc.to_step(NR.delete_tags(c["steps"][i], keep)))
    plain = dev.solve_batch(deleted, [c["gyro"][i] for i in planted])
    for i, d in zip(planted, plain):
        g, label = got[i], f"{name}[{i}]"
        masks = [int(m) for m in g["rejected"]]
        if masks != c["planted"][i] + [0] * (len(masks) - c["n_cams"]):
            rc._fail(label, "rejected", [hex(m) for m in masks], [hex(m) for m in c["planted"][i]])
        assert g["status"] == A.CK_RIG_ROBUST_REJECTED and g["n_rejected"] == sum(bin(m).count("1") for m in c["planted"][i]), label
        rc.fused_against_twin(label + " fused vs the plain solve without the planted tags", g["fused"], d)


def test_clean_robust_step_is_the_plain_record(dev, solved):
    """64, 128 and 512 tags without an outlier: `fused` is k_rig's record, byte for byte"""
    for name, i, n_tags in (("count_one_camera_robust", 7, 64), ("count_bit63_robust", 1, 128), ("count_full_robust", 1, 512)):
        c = rc.case(name)
        got = solved(name)[i]
        plain = dev.solve_batch([rc.to_step(c["steps"][i])], [c["gyro"][i]])[0]
        assert plain["valid"] == 1 and plain["n_tags"] == n_tags
        assert (got["status"], got["rounds"], got["n_rejected"]) == (A.CK_RIG_ROBUST_CLEAN, 0, 0) and not got["rejected"].any(), name
        if got["fused"].tobytes() != plain.tobytes():
            rc._fail(f"{name}[{i}]", "fused (bytes)", got["fused"].tolist(), plain.tolist())


def test_batch_position_does_not_matter(dev, solved):
    """count_one_camera in order and reversed, an empty step between each pair: a record's bytes depend on its step alone"""
    c = rc.case("count_one_camera")
    base = solved("count_one_camera")
    empty = rc.empty_like(c["steps"][0])
    for order in (list(range(len(c["steps"]))), list(range(len(c["steps"])))[::-1]):
        steps, gyro, where = [], [], {}
        for k, i in enumerate(order):
            if k:
                steps.append(rc.to_step(empty)); gyro.append(0.0)
            where[i] = len(steps)
            steps.append(rc.to_step(c["steps"][i])); gyro.append(c["gyro"][i])
        got = dev.solve_batch(steps, gyro)
        for i, at in where.items():
            if got[at].tobytes() != base[i].tobytes():
                rc._fail(f"count_one_camera[{i}] at position {at}", "record (bytes)", got[at].tolist(), base[i].tolist())
        for at in set(range(len(steps))) - set(where.values()):
            assert got[at].tobytes() == bytes(got[at].nbytes), at


def test_determinism(dev, solved):
    for name in ("count_full", "count_full_robust"):
        again = rc.solve(dev, rc.case(name))
        assert again.tobytes() == solved(name).tobytes(), name
    assert solved("count_full")["valid"].all() and solved("count_full_robust")["n_rejected"][0] == 8


def test_robust_call_refuses_65_tags(dev):
    """65 tags in a camera are more than a mask has bits: CK_EINVAL, the handle stays usable and the plain call solves the input"""
    c = rc.case("count_full")
    steps, gyro = [rc.to_step(c["steps"][1])], [c["gyro"][1]]
    with pytest.raises(ChalkydriError) as e:
        dev.solve_batch(steps, gyro, robust=True)
    assert e.value.code == A.CK_EINVAL
    got = dev.solve_batch(steps, gyro)[0]
    assert got["valid"] == 1 and got["n_tags"] == 520 and list(got["cam_tags"]) == [65] * 8
