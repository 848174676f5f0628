"""The front half of the quad fit (bounding box, border direction, sort, duplicate removal) at the edges of its size classes, on both
paths of the sort, in both kernels: k_fit (a call of a few frames on the product library, in this process) and k_seq (the split fit,
forced for every call by CK_FIT_FLAT=2 on the diagnostics build, in a child process: tests/seq_front_child.py).  Bit-exact against
the oracle; the inputs are drawn here and the conditions they have to meet are asserted on the oracle's clusters, on the CPU, before
the device is asked for anything."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# class edge (points per cluster) -> threads per cluster of the class below it (k_quads.hip: FIT_CLASS); "near" an edge = within that many
EDGES = {256: 64, 512: 64, 1024: 128, 2048: 256, 4096: 256}


def _nested(w, h, sides, cx, cy, skew, rings=()):
    """Filled, slightly skewed quadrilaterals inside each other, alternating bright and dark, on a flat background: one gradient
    cluster per outline, of about 12.3 points per pixel of side (the skew makes diagonal steps, whose points come twice).  rings:
    (cx, cy, r) annuli, two outlines each of about 19.3 r and 15.4 r points."""
    im = np.full((h, w), 40, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for k, s in enumerate(sides):
        im[(np.abs((xx - cx) - skew * (yy - cy)) < s / 2) & (np.abs(yy - cy) < s / 2)] = 215 if k % 2 == 0 else 40
    for rx, ry, r in rings:
        rr = np.hypot(xx - rx, yy - ry)
        im[(rr < r) & (rr > 0.8 * r)] = 215
    return im


def _shapes(w, h, seed):
    """Hand-drawn frame that drives the sort of every size class through both of its paths: thin bars and spokes put
    hundreds of boundary points into one angle bucket (bitonic fallback), blobs and rings spread them out (bucket path);
    the outline rectangles are large-class clusters.  (The generator of tests/test_gpu_detect.py, copied.)"""
    rng = np.random.default_rng(seed)
    im = np.full((h, w), 40, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    im[20:23, 30:w - 40] = 220                                  # long thin bars
    im[40:h - 30, 14:17] = 220
    im[(np.abs((yy - 60) - (xx - 40) * 0.31) < 1.6) & (xx > 40) & (xx < w - 60)] = 220   # thin slanted line
    im[60:h - 20, 60:w - 20] = 215                              # big plate ...
    im[70:h - 30, 70:w - 30] = 35                               # ... hollowed: two long outlines
    cx, cy = w // 2, h // 2 + 10
    r = np.hypot(xx - cx, yy - cy)
    im[(r < 0.28 * h) & (r > 0.2 * h)] = 225                    # ring
    for k in range(12):                                         # spokes inside the ring
        a = k * np.pi / 6 + 0.1
        d = np.abs((xx - cx) * np.sin(a) - (yy - cy) * np.cos(a))
        im[(d < 1.3) & (r < 0.18 * h) & (r > 6)] = 225
    for _ in range(10):                                         # filled quadrilaterals of assorted sizes
        x0, y0 = rng.integers(80, w - 160), rng.integers(80, h - 120)
        sw, sh = rng.integers(14, 70), rng.integers(14, 70)
        sk = rng.uniform(-0.4, 0.4)
        m = (np.abs((xx - x0) - sk * (yy - y0)) < sw / 2) & (np.abs(yy - y0) < sh / 2)
        im[m] = 228 if rng.random() < 0.5 else 20
    noise = rng.integers(-1, 2, im.shape)
    return np.clip(im.astype(np.int64) + noise, 0, 255).astype(np.uint8)


def _frames():
    """name -> frames of one call.  The sides are swept around 12.3 points per pixel so that the outlines' point counts lie just
    below (first frame) and just above (second frame) 256, 512, 1024, 2048 and 4096."""
    below, above = (330, 164, 82, 42, 21), (344, 176, 88, 44, 23)
    e640 = np.stack([_nested(640, 480, below, 196, 240, 0.15, rings=((520, 130, 105), (520, 360, 52))),
                     _nested(640, 480, above, 200, 240, 0.15, rings=((520, 130, 112), (520, 360, 56)))])
    e272 = np.stack([_nested(272, 200, below[1:], 120, 100, 0.12), _nested(272, 200, above[1:], 124, 100, 0.12)])
    s640 = np.stack([_shapes(640, 480, 1), _shapes(640, 480, 11)[::-1].copy()])
    # more frames than a call may bring and still have its classes run side by side (16): the batch plan, with the two youngest
    # classes (up to 256 and 513..1024 points) that small calls do without
    batch = np.concatenate([e640, s640] * 4 + [e640])
    return {"edges640": e640, "edges272": e272, "shapes640": s640, "batch640": batch}


def _cluster_sizes(oracle, frame):
    """(points, points left after duplicate removal) of every cluster of the frame, from the oracle"""
    th = oracle.threshold(frame)
    lab, sz = oracle.segment(th)
    cl, pts, _ = oracle.clusters(th, lab, sz)
    out = []
    for _, _, start, count in cl:
        p = pts[start:start + count]
        out.append((int(count), len(np.unique(p["x"].astype(np.int64) << 16 | p["y"].astype(np.int64)))))
    return cl, pts, out


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """The frames, the oracle's quads of every distinct frame (computed once, shared by all tests) and its cluster sizes."""
    from chalkydri_amd import default_config
    data, sizes, nquads = {}, {}, {}
    for name, frames in _frames().items():
        n, h, w = frames.shape
        cfg = default_config(w, h)
        uniq, index = [], []
        for i in range(n):   # a frame that repeats an earlier one of the call shares its oracle result
            j = next((u for u in uniq if np.array_equal(frames[u], frames[i])), None)
            if j is None:
                uniq.append(i); j = i
            index.append(j)
        sizes[name], nquads[name] = [], 0
        for i in uniq:
            cl, pts, sz = _cluster_sizes(oracle, frames[i])
            q = oracle.quads_to_np(oracle.fit_quads(frames[i], cfg, cl, pts)[0])
            data["q_%s_%d" % (name, i)] = q[np.lexsort((q[:, 10], q[:, 9]))] if len(q) else q
            sizes[name] += sz
            nquads[name] += len(q)
        data["f_" + name], data["u_" + name] = frames, np.asarray(index)
    path = str(tmp_path_factory.mktemp("seq_front") / "cases.npz")
    np.savez(path, **data)
    return path, data, sizes, nquads


def _assert_inputs(sizes, nquads):
    """Conditions on the inputs, checked on the oracle's clusters: without them the tests could pass without having run the code."""
    for name in ("edges640", "edges272"):
        counts = [c for c, _ in sizes[name]]
        for edge, nth in EDGES.items():
            if edge == 4096 and name == "edges272":
                continue   # 3 * (2 * 272 + 2 * 200) = 2 832 points at most in such a frame
            assert any(edge - nth < c <= edge for c in counts), f"{name}: no cluster just below {edge}: {sorted(counts)}"
            assert any(edge < c <= edge + nth for c in counts), f"{name}: no cluster just above {edge}: {sorted(counts)}"
        assert any(u != c for c, u in sizes[name]), f"{name}: no cluster with duplicate points"
        assert nquads[name] >= 4
    counts = [c for c, _ in sizes["shapes640"]]
    assert any(c <= 512 for c in counts) and any(512 < c <= 4096 for c in counts) and any(4096 < c for c in counts)
    assert nquads["shapes640"] >= 3


def test_inputs_straddle_every_class_edge(cases):
    _, _, sizes, nquads = cases
    _assert_inputs(sizes, nquads)


@pytest.mark.parametrize("name", ["edges640", "edges272", "shapes640", "batch640"])
def test_front_half_in_k_fit(cases, name):
    """In this process, on the product library: calls this small run the unsplit fit, k_fit."""
    from chalkydri_amd.detector import AprilTagDetector
    _, data, sizes, nquads = cases
    _assert_inputs(sizes, nquads)
    frames = data["f_" + name]
    n, h, w = frames.shape
    det = AprilTagDetector(w, h, max_batch=n)
    got = det.quads(frames)
    det.close()
    bad = []
    for i in range(n):
        a = oracle_np(got[i])
        want = data["q_%s_%d" % (name, int(data["u_" + name][i]))]
        if a.shape != want.shape or not np.array_equal(a, want):
            bad.append((i, len(a), len(want)))
    assert not bad, f"frames that differ from the oracle (frame, device quads, oracle quads): {bad}"


def oracle_np(quads):
    import pyoracle
    a = pyoracle.quads_to_np(quads)
    return a[np.lexsort((a[:, 10], a[:, 9]))] if len(a) else a


def _child(path):
    """The cases in a child process on the diagnostics build with the split fit forced: k_seq -> k_chunk -> k_tail.  The child's
    GPU work runs under a time limit of its own."""
    from conftest import diag_env
    env = diag_env(CK_FIT_FLAT="2")   # (a knob of the diagnostics build)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "seq_front_child.py"), path], capture_output=True,
                       text=True, env=env, timeout=300)
    lines = r.stdout.splitlines()
    bad = [ln for ln in lines if ln.startswith("MISMATCHING_FRAMES")]
    hashes = [ln for ln in lines if ln.startswith("HASH")]
    assert bad and hashes, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return int(bad[0].split()[1]), hashes[0].split()[1], r


@pytest.fixture(scope="module")
def child_runs(cases):
    """two runs of the child on the same file (one for parity, both for determinism)"""
    return [_child(cases[0]) for _ in range(2)]


def test_front_half_in_k_seq(cases, child_runs):
    _assert_inputs(cases[2], cases[3])
    bad, _, r = child_runs[0]
    assert bad == 0 and r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_split_fit_is_deterministic(child_runs):
    """The same calls in a second process: identical quads (the clusters that gave one included) and status words."""
    assert child_runs[0][1] == child_runs[1][1]
    assert child_runs[1][0] == 0
