"""The split quad fit's moment prefix sums (k_chunk files the running sums of every span at its block ends; k_tail takes a target's
prefix from one entry plus the totals of the spans between the cluster's first and the target's): clusters that touch three spans
and more, sequences that cross many span boundaries, and the same on poisoned buffers.  Every case is a child process on the
diagnostics build with CK_FIT_FLAT=2 (the split fit on every call); its quads must be the oracle's bit for bit."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN = 960   # CK_SPAN: positions one k_chunk workgroup decides

CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import pyoracle
from chalkydri_amd.detector import AprilTagDetector
z = np.load(sys.argv[1])
frames, runs = z["frames"], int(sys.argv[2])
n, h, w = frames.shape
det = AprilTagDetector(w, h, max_batch=n)
bad = 0
for r in range(runs):   # one handle: where a sequence lands follows an atomic counter, so its span and block alignment differs from run to run
    got = det.quads(frames)
    for i in range(n):
        a = pyoracle.quads_to_np(got[i])
        a = a[np.lexsort((a[:, 10], a[:, 9]))] if len(a) else a
        want = z["q%%d" %% i]
        if a.shape != want.shape or not np.array_equal(a, want):
            bad += 1
            print("MISMATCH run", r, "frame", i, "have", len(a), "want", len(want))
det.close()
print("CHECKED", runs * n, "BAD", bad)
"""


def _H(cx, cy, side, deg):
    a, c, s = side / 2.0, math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [[a * c, -a * s, cx], [a * s, a * c, cy], [0.0, 0.0, 1.0]]


def _sequence_sizes(oracle, frame, cfg):
    """Points of the extended sequences k_seq hands to k_chunk for this frame, per cluster: fit_quad's rejections before the sort
    (oracle/detector.c: size, bounding box, border direction — tag36h11 takes normal borders only) and its duplicate removal.
    The library's C interface does not hand out the device's per-frame position counter, so the tests bound it from below on the
    oracle's clusters, which the device's equal bit for bit: the counter is the sum of these sizes plus 49 positions per cluster."""
    th = oracle.threshold(frame, cfg.min_white_black_diff)
    lab, sz = oracle.segment(th)
    cl, pts, _ = oracle.clusters(th, lab, sz, cfg.min_component_px)
    out = []
    for _, _, start, count in cl:
        if count < max(24, cfg.min_cluster_pixels):
            continue
        p = pts[start:start + count]
        x, y = p["x"].astype(np.int64), p["y"].astype(np.int64)
        if (x.max() - x.min()) * (y.max() - y.min()) < 8:   # min_tag_width: tag36h11's width at the border
            continue
        if np.sum((4 * x - 2 * (x.min() + x.max()) - 1) * p["gx"] + (4 * y - 2 * (y.min() + y.max()) + 1) * p["gy"]) < 0:
            continue
        n = len(np.unique(x << 16 | y))
        if n >= 24:
            out.append(n)
    return out


def _large_tag_frames():
    """One tag of side 300 px (its outline alone is a cluster of well over two spans) and four of 30-60 px beside it."""
    from chalkydri_amd import synth
    tags = [(0, 7, _H(200, 240, 300, 4)), (0, 11, _H(470, 70, 40, -8)), (0, 23, _H(575, 95, 56, 12)), (0, 42, _H(480, 300, 32, 20)),
            (0, 99, _H(575, 380, 60, -15))]
    return synth.render_scene(1234, 640, 480, tags)[0][None]


def _span_boundary_frames():
    """Four frames of 320x240 with eight tags of side 40-100 px on the bench's background (ramp, noise +-3): the noise supplies the
    clusters that carry a frame's sequences over several span boundaries (some 7 000 positions per frame)."""
    from chalkydri_amd import synth
    lay = [(68, 68, 100), (50, 190, 64), (125, 200, 48), (180, 50, 56), (255, 40, 40), (285, 110, 44), (205, 170, 72), (290, 200, 40)]
    frames = []
    for i in range(4):
        tags = [(0, 10 * i + k, _H(cx + i, cy + (i & 1), side, 2 * i - 3 + (k & 1))) for k, (cx, cy, side) in enumerate(lay)]
        frames.append(synth.render_scene(500 + i, 320, 240, tags, noise_amp=3)[0])
    return np.stack(frames)


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """name -> (file with the frames and the oracle's quads, sequence sizes per frame); computed once for all tests."""
    from chalkydri_amd import default_config
    out = {}
    for name, frames in (("large", _large_tag_frames()), ("spans", _span_boundary_frames())):
        n, h, w = frames.shape
        cfg = default_config(w, h)
        data = {"frames": frames}
        for i in range(n):
            q = oracle.quads_to_np(oracle.quads(frames[i], cfg))
            data["q%d" % i] = q[np.lexsort((q[:, 10], q[:, 9]))] if len(q) else q
        path = str(tmp_path_factory.mktemp("tail_prefix") / (name + ".npz"))
        np.savez(path, **data)
        out[name] = (path, [_sequence_sizes(oracle, frames[i], cfg) for i in range(n)], [len(data["q%d" % i]) for i in range(n)])
    return out


def _child(path, runs, poison):
    from conftest import diag_env
    env = diag_env(CK_FIT_FLAT="2")   # (a knob of the diagnostics build)
    if poison:
        env["CK_POISON"] = "1"        # the handle's buffers start as 0xA5 bytes: an entry read without having been written shows
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "oracle")), path, str(runs)], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("poison", [False, True])
def test_one_large_tag_beside_small_ones(cases, poison):
    path, sizes, nquads = cases["large"]
    assert max(sizes[0]) > 2 * SPAN          # a condition on the input: some cluster touches three spans or more
    assert nquads[0] >= 5                    # the five tags' quads are among the oracle's
    out = _child(path, 8, poison)
    assert "CHECKED 8 BAD 0" in out, out[-2000:]


@pytest.mark.parametrize("poison", [False, True])
def test_sequences_across_span_boundaries(cases, poison):
    path, sizes, nquads = cases["spans"]
    assert max(sum(s) for s in sizes) > 2 * SPAN   # a condition on the input: a frame's sequences fill more than two spans
    assert min(nquads) >= 8
    out = _child(path, 2, poison)
    assert "CHECKED 8 BAD 0" in out, out[-2000:]
