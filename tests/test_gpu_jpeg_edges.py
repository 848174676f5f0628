"""k_jpeg_frame at its own edges ("The entropy decoder at its own edges"): the batches of tests/jpeg_edge_cases.py,
whose conditions (which synchronisation path, stale and empty pieces, the cap, where the unstuffer's pairs fall, ...) are asserted on
the CPU by measure() before the device is asked for anything.  Luma bytes and status words equal tests/np_jpeg.py's, a failed
frame is zeros and its neighbours are exact; the same batches through ck_upload_jpeg_color (triples against tests/np_jpeg_color.py),
through ring slots, and in a child process on the diagnostics build, plain and on poisoned buffers.  Every comparison is byte
equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_edge_cases as EC  # noqa: E402
import jpeg_edges_child as child  # noqa: E402
import np_jpeg as J  # noqa: E402
import np_jpeg_color as JC  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_FAMILIES = ("tails", "pieces")
RING_FAMILIES = ("paths", "tails")

_batches = {}


def batch(fam):
    """(streams, expected luma, expected status) of a family: measured (and its conditions asserted) once"""
    if fam not in _batches:
        _batches[fam] = EC.batch(fam)
    return _batches[fam]


@pytest.mark.parametrize("fam", EC.FAMILIES)
def test_luma_and_status(built, fam):
    """One call per family, twice on one handle, and the luma the colour form stages."""
    streams, want, want_st = batch(fam)
    assert all(not want[i].any() for i in range(len(streams)) if want_st[i] != J.OK)
    bad = child.run_family(streams, want, want_st)
    names = EC.names(fam)
    assert not bad, "%s: (call, case, what) %s" % (fam, [(c, names[i], what) for c, i, what in bad[:12]])


@pytest.mark.parametrize("fam", EC.FAMILIES)
def test_colour_form_keeps_the_chroma(built, fam):
    """ck_upload_jpeg_color, the COLOR instantiation of the same kernel: status words, and the (Y, Cb, Cr) triples at identity size
    equal the restatement's (failed frames (0, 128, 128)); a second call on the handle gives the same bytes."""
    from chalkydri_amd.detector import AprilTagDetector
    streams, want, want_st = batch(fam)
    n, (w, h) = len(streams), EC.SIZES[fam]
    det = AprilTagDetector(w, h, max_batch=n)
    first = None
    for _ in range(2):
        k, st = det.upload_jpeg(streams, return_status=True, color=True)
        assert k == n and st == want_st
        got = det.preview_color(list(range(n)), width=0, height=0)
        assert got.shape == (n, h, w, 3)
        if first is None:
            first = got.copy()
            for i, name in enumerate(EC.names(fam)):
                C, cst = JC.decode_color(streams[i], (w, h))
                assert cst == want_st[i] and np.array_equal(C[..., 0], want[i]), name
                assert np.array_equal(got[i], C), (name, int((got[i] != C).any(axis=-1).sum()))
        else:
            assert np.array_equal(got, first)
    det.close()


@pytest.mark.parametrize("fam", RING_FAMILIES)
def test_ring_slots(built, fam):
    """The fixed layout of a ring slot (sized once for max_frame_bytes): a ring of ck_ingest_create_jpeg gives the status words and
    the detections of the plain upload; a ring of ck_ingest_create_jpeg_color, the same slots with the planes kept, gives the
    triples of the plain colour upload, which test_colour_form_keeps_the_chroma holds against the restatement.  Each slot twice."""
    from chalkydri_amd.detector import AprilTagDetector, IngestRing
    streams, want, want_st = batch(fam)
    n, (w, h) = len(streams), EC.SIZES[fam]
    det = AprilTagDetector(w, h, max_batch=n)
    det.upload_jpeg(streams)
    key = lambda dets: [[(d.id(), d.corners().tobytes()) for d in f] for f in dets]  # noqa: E731
    want_dets = key(det.detect_batch(None, n=n))
    det.upload_jpeg(streams, color=True)
    triples = det.preview_color(list(range(n)), width=0, height=0).copy()
    assert all(np.array_equal(triples[i, ..., 0], want[i]) for i in range(n))
    cap = max(len(b) for b in streams)
    for color in (False, True):
        ring = IngestRing(det, 1, fourcc="MJPG", max_frame_bytes=cap, color=color)
        for _ in range(2):
            for i, b in enumerate(streams):
                ring.write(0, i, b)
            ring.submit(0, n)
            assert ring.jpeg_status(0, n) == want_st
            if color:
                assert np.array_equal(ring.preview_color(0, list(range(n)), width=0, height=0), triples)
            dets, _ = ring.detect(0, n)
            assert key(dets) == want_dets
        ring.close()
    det.close()


def _child(path, **knobs):
    """The child on the diagnostics build; its GPU work runs under a time limit of its own."""
    from conftest import diag_env
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(HERE, "jpeg_edges_child.py"), path], capture_output=True,
                       text=True, env=diag_env(**knobs), timeout=180)
    lines = r.stdout.splitlines()
    bad = [ln for ln in lines if ln.startswith("MISMATCHING_FAMILIES")]
    hashes = [ln for ln in lines if ln.startswith("HASH")]
    assert bad and hashes, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return int(bad[0].split()[1]), hashes[0].split()[1], r


@pytest.fixture(scope="module")
def child_runs(built, tmp_path_factory):
    """two runs of the child on the same file: plain, and with every device buffer starting as 0xA5 bytes"""
    path = str(tmp_path_factory.mktemp("jpeg_edges") / "batches.npz")
    np.savez(path, **child.pack({fam: batch(fam) for fam in CHILD_FAMILIES}))
    plain = _child(path)
    if plain[2].returncode not in (0, 1):   # (ended by a signal or its time limit: nothing more is started on the device)
        return [plain, plain]
    return [plain, _child(path, CK_POISON="1")]


def test_tails_and_pieces_on_the_diagnostics_build(child_runs):
    bad, _, r = child_runs[0]
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_tails_and_pieces_on_poisoned_buffers(child_runs):
    """A stale or unwritten piece record that is read would show as bytes that differ."""
    assert child_runs[1] is not child_runs[0], "the plain run did not end by itself"
    bad, h, r = child_runs[1]
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert h == child_runs[0][1]
