"""GPU: the detector on the test families of tests/family_gen.py (reversed borders, odd bit counts, bits outside the border,
64-bit code words, four families in one handle) — bit-exact with the oracle, and right against the ground truth of
tests/np_tag_render.py and the numpy decoder of tests/np_at3_decode.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import family_gen as fg
import np_tag_render
import quad_filter_ref
import stress_families
from chalkydri_amd import default_config, family
from chalkydri_amd.detector import AprilTagDetector
from test_family_decode import MAX_HAMMING, _pairs_with_oracle, check_truth
from test_gpu_detect import _same_dets

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _frames(fams, seed, n, w, h, **kw):
    out = [np_tag_render.scene(fams, seed + i, w=w, h=h, **kw) for i in range(n)]
    return np.stack([f for f, _ in out]), [t for _, t in out]


@pytest.mark.parametrize("w,h", [(643, 481), (642, 479)])
@pytest.mark.parametrize("dec", [1, 2])
@pytest.mark.parametrize("name", list(fg.MATRIX))
def test_detect_matches_oracle_and_truth(oracle, name, dec, w, h):
    f = fg.make(name)
    mh = MAX_HAMMING.get(name, 3)
    n = 2
    frames, truths = _frames([f], 300 + 10 * dec + w % 2, n, w, h)
    det = AprilTagDetector(w, h, max_batch=n, families=(f,), quad_decimate=dec, bits_corrected=mh)
    got, status = det.detect_batch(frames, return_status=True)
    det.close()
    cfg = default_config(w, h, families=(f,), quad_decimate=dec, max_hamming=mh)
    for i in range(n):
        want, st = oracle.detect(frames[i], cfg)
        assert status[i] == st == 0
        _same_dets(got[i], want)
        check_truth(want, truths[i])
        assert _pairs_with_oracle(oracle, frames[i], cfg, [f]) >= len(truths[i])


FOUR = ("tag36h11", "std41r", "circ21r", "full64")


@pytest.mark.parametrize("dec,sigma", [(1, 0.0), (2, 0.0), (1, 0.8)])
def test_four_families_in_one_handle(oracle, dec, sigma):
    fams = tuple(family(n) if n.startswith("tag") else fg.make(n) for n in FOUR)
    w, h, n = 961, 641, 2
    frames, truths = _frames(list(fams), 70 + dec, n, w, h, cols=4, rows=3)
    det = AprilTagDetector(w, h, max_batch=n, families=fams, quad_decimate=dec, bits_corrected=2, quad_sigma=sigma)
    got, status = det.detect_batch(frames, return_status=True)
    det.close()
    cfg = default_config(w, h, families=fams, quad_decimate=dec, max_hamming=2)
    kinds = set()
    for i in range(n):
        if sigma:   # the oracle on the filtered quad image (quad_decimate 1: edge refinement and decode read it too)
            want, st = oracle.detect(quad_filter_ref.quad_image(frames[i], sigma, 1), cfg)
        else:
            want, st = oracle.detect(frames[i], cfg)
            check_truth(want, truths[i])
        assert status[i] == st
        _same_dets(got[i], want)
        kinds |= {d.family() for d in got[i]}
    assert kinds == {0, 1, 2, 3}


@pytest.mark.parametrize("names,dec", stress_families.QUAD_CASES)
def test_quads_match_oracle_with_reversed_borders(oracle, names, dec):
    """ck_quads_batch equals the oracle's quads for a reversed-only configuration (every quad reversed) and a mixed one."""
    bad, flags, fewest = stress_families.quad_parity(names, dec)
    assert bad == 0 and fewest >= 12
    assert flags == ({1} if all(fg.MATRIX.get(n, (0, 0, 0, 0))[3] for n in names) else {0, 1})


def test_quads_match_oracle_with_reversed_borders_split_fit():
    """The same quad comparisons through the split quad fit (k_seq -> k_chunk -> k_tail): CK_FIT_FLAT=2 of the diagnostics build, in
    a child (the knob is read once per process)."""
    from conftest import diag_env
    env = diag_env(CK_FIT_FLAT="2")   # (a knob of the diagnostics build)
    r = subprocess.run([sys.executable, os.path.join(HERE, "stress_families.py"), "--quads"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '"quad_mismatching_frames": 0' in r.stdout, r.stdout[-2000:]


def test_stress_families_small_dose():
    r = subprocess.run([sys.executable, os.path.join(HERE, "stress_families.py"), "25", "5"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '"mismatching_frames": 0' in r.stdout, r.stdout[-2000:]


def test_stress_families_split_fit():
    """The split quad fit (k_seq -> k_chunk -> k_tail) on the same cases: CK_FIT_FLAT=2 of the diagnostics build, in a child."""
    from conftest import diag_env
    env = diag_env(CK_FIT_FLAT="2")   # (a knob of the diagnostics build)
    r = subprocess.run([sys.executable, os.path.join(HERE, "stress_families.py"), "25", "6"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '"mismatching_frames": 0' in r.stdout, r.stdout[-2000:]
