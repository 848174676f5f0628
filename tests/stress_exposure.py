"""Random exposure-metering cases against the numpy restatement (tests/np_exposure.py):  python tests/stress_exposure.py N SEED
Every case draws a size 16..700 (ragged), a batch of 1..6 frames of mixed content (noise of several amplitudes, flat, ramps, tag
scenes' texture), gamma curves, a frame list with repeats and a rectangle per entry (inside, across a border, empty, none), and
compares ck_exposure_stats byte for byte.  One JSON line."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import np_exposure as N  # noqa: E402


def content(rng, w, h):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return np.full((h, w), int(rng.integers(0, 256)), np.uint8)
    if kind == 1:
        amp = int(rng.choice([1, 2, 4, 16, 64]))
        return np.clip(int(rng.integers(0, 256)) + rng.integers(-amp, amp + 1, (h, w)), 0, 255).astype(np.uint8)
    if kind == 2:
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == 3:
        yy, xx = np.mgrid[0:h, 0:w]
        return ((xx * int(rng.integers(1, 9)) + yy * int(rng.integers(0, 5))) & 255).astype(np.uint8)
    cell = int(rng.integers(2, 40))
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // cell) + (xx // cell)) % 2 == 0, int(rng.integers(0, 128)), int(rng.integers(128, 256))).astype(np.uint8)


def rect(rng, w, h):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return (0, 0, w, h)
    if kind == 1:
        return (-int(rng.integers(0, 50)), -int(rng.integers(0, 50)), w + int(rng.integers(0, 50)), h + int(rng.integers(0, 50)))
    if kind == 2:
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        return (x, y, x, y + 3)
    x0, x1 = sorted(int(v) for v in rng.integers(-8, w + 9, 2))
    y0, y1 = sorted(int(v) for v in rng.integers(-8, h + 9, 2))
    return (x0, y0, x1, y1)


def run(n_cases, seed, verbose=False):
    from chalkydri_amd.detector import AprilTagDetector
    from chalkydri_amd.exposure import ExposureParams
    rng = np.random.default_rng(seed)
    mismatching, n_frames = [], 0
    for case in range(n_cases):
        w, h, n = int(rng.integers(16, 701)), int(rng.integers(16, 701)), int(rng.integers(1, 7))
        frames = np.stack([content(rng, w, h) for _ in range(n)])
        p = ExposureParams() if case % 3 == 0 else ExposureParams(gamma=np.cumsum(rng.uniform(0.05, 0.8, 7)))
        lut = p.luts()
        m = int(rng.integers(1, 7))
        idx = [int(v) for v in rng.integers(0, n, m)]
        rois = None if case % 4 == 0 else [rect(rng, w, h) for _ in range(m)]
        det = AprilTagDetector(w, h, max_batch=6)
        det.upload(frames)
        got = det.exposure_stats(frames=idx, roi=rois, params=p)
        det.close()
        bad = sum(got[i].tobytes() != N.stats(frames[f], lut, None if rois is None else rois[i]).tobytes() for i, f in enumerate(idx))
        n_frames += m
        if bad:
            mismatching.append({"case": case, "w": w, "h": h, "records": bad})
        if verbose:
            print(case, w, h, n, idx, rois, bad, flush=True)
    return {"cases": n_cases, "seed": seed, "frames": n_frames, "mismatching": len(mismatching), "first": mismatching[:5]}


if __name__ == "__main__":
    out = run(int(sys.argv[1]) if len(sys.argv) > 1 else 100, int(sys.argv[2]) if len(sys.argv) > 2 else 1, verbose=len(sys.argv) > 3)
    print(json.dumps(out))
    sys.exit(1 if out["mismatching"] else 0)
