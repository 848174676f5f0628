"""The decode stage (k_decode, k_finalize) at its own edges, detection for detection, through ck_decode_quads_batch: the codebook
search beyond one pass of 768 codes, its tie rule, samples outside the frame, non-finite sample coordinates, gray models that cannot
be solved, a margin of exactly 0, more candidates than k_finalize has threads, det_cap, equal candidates, zero cross products, and
the batch.  Equality of bytes against the oracle (id, hamming, family, float margin, centre, corners), of counts and of status; the
cases are tests/decode_cases.py's, and tests/test_decode_cases_host.py proves on the CPU that they reach what they name."""
import os
import subprocess
import sys

import pytest

import decode_cases as dc
from chalkydri_amd import _abi as A

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", dc.NAMES)
def test_decode_equals_the_oracle(oracle, name):
    """from host frames and on the staged frames; where a truth exists, the drawn id and corners (dc.check_truth)"""
    bad, _, _ = dc.run_case(dc.detector, oracle, name)
    assert not bad, bad


@pytest.mark.parametrize("name", ["finalize_counts", "finalize_dups", "finalize_edge", "finalize_nan", "finalize_two_families", "batch_plain", "overhang_odd"])
def test_order_of_the_quads_does_not_show(oracle, name):
    """the quad lists shuffled between two calls: the candidates arrive in another order, the bytes are the same"""
    bad, first, _ = dc.run_case(dc.detector, oracle, name)
    bad2, second, _ = dc.run_case(dc.detector, oracle, name, shuffle=5)
    assert not bad and not bad2 and first == second


def test_status_carries_decode_bits_only(oracle):
    """257 tags: CK_FRAME_DETS_OVERFLOW and exactly the first 256 of the order; ids 39, 40: CK_FRAME_UNVERIFIED_ID; the caller's cap"""
    c = dc.case("finalize_counts")
    det = dc.detector(dc.FIN_W, dc.FIN_H, 4, c["settings"])
    got, status = det.decode_quads(c["quads"], c["frames"], cap=dc.DET_CAP, return_status=True)
    det.close()
    unv, ovf = A.CK_FRAME_UNVERIFIED_ID, A.CK_FRAME_DETS_OVERFLOW   # (ids from 39 on are past the built-in family's upstream prefix)
    assert status == [unv, unv, unv | ovf, unv | ovf]
    assert [[d.id() for d in fr] for fr in got] == [list(range(min(n, 256))) for n in dc.FIN_COUNTS]
    c = dc.case("finalize_dups")
    det = dc.detector(256, 160, 2, c["settings"])
    _, status = det.decode_quads(c["quads"], c["frames"], return_status=True)
    one, st1 = det.decode_quads([c["quads"][1][:1]], c["frames"][1:], return_status=True)   # id 38 alone: the last upstream id
    det.close()
    assert status == [0, A.CK_FRAME_UNVERIFIED_ID] and st1 == [0] and [d.id() for d in one[0]] == [38]
    c = dc.case("finalize_two_families")
    det = dc.detector(256, 120, 1, c["settings"])
    got, status = det.decode_quads(c["quads"], c["frames"], cap=5, return_status=True)
    det.close()
    assert len(got[0]) == 5 and status == [ovf | unv]   # (12 detections for a cap of 5; ids 40..42 are among them)


def test_decode_after_a_detect_and_before_one(oracle):
    """the entry point leaves nothing behind that the next pipeline run reads, and reads nothing the last one left: detect, decode the
    caller's quads, detect again on one handle"""
    c = dc.case("batch_plain")
    frames = c["frames"]
    det = dc.detector(frames.shape[2], frames.shape[1], c["max_batch"], c["settings"])
    key = lambda rs: [[(d.id(), d.hamming(), d.corners().tobytes()) for d in fr] for fr in rs]
    before = key(det.detect_batch(frames))
    got, status = det.decode_quads(c["quads"], frames, return_status=True, raw=True)
    after = key(det.detect_batch(frames))
    det.close()
    want, _ = dc.expected(oracle, c)
    assert [(g, len(g) // 96, s) for g, s in zip(got, status)] == want and before == after


def _child(shuffle, **env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "decode_child.py"), str(shuffle)], capture_output=True,
                       text=True, env=env, timeout=300)
    lines = r.stdout.splitlines()
    bad = [ln for ln in lines if ln.startswith("MISMATCHING_CASES")]
    hashes = [ln for ln in lines if ln.startswith("HASH")]
    assert bad and hashes, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return int(bad[0].split()[1]), hashes[0].split()[1], r


def test_decode_on_poisoned_buffers(oracle):
    """Every case in a child process whose handles' buffers start as 0xA5 bytes, the quad lists shuffled: an entry read without having been
    written (a quad slot past the count, a candidate count, a counter) would show as a detection that differs."""
    bad, _, r = _child(9, CK_POISON="1")
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_largest_accepted_quad_capacity(oracle):
    """one detect and one decode at max_quads_per_frame = CK_MAX_FRAME_CANDIDATES: k_finalize's launch with 64 KiB of dynamic LDS"""
    c = dc.case("batch_plain")
    settings = dict(c["settings"], max_quads_per_frame=16384)
    frames = c["frames"]
    h, w = frames.shape[1:]
    det = dc.detector(w, h, 3, settings)
    dets = det.detect_batch(frames)
    got, status = det.decode_quads(c["quads"], frames, return_status=True, raw=True)
    det.close()
    want, _ = dc.expected(oracle, c)
    assert [(g, len(g) // 96, s) for g, s in zip(got, status)] == want
    cfg = dc.config(w, h, settings)
    for i in range(3):
        o, _ = oracle.detect(frames[i], cfg)
        assert [(d.id(), d.corners().tobytes()) for d in dets[i]] == [(d["id"], d["p"].tobytes()) for d in o]
