"""Randomised parity stress of the device JPEG decode: random sizes 16..400, every sampling and grey, restart intervals (none, 1..9
MCUs, whole MCU rows), quality 1..100, smooth or noise content, standard / shuffled / absent Huffman tables, 8- or 16-bit DQT; the
luma and status of every frame must equal the numpy restatement of libjpeg (tests/np_jpeg.py).  One detector per case, a batch
of 1..4 streams of its geometry.  Prints one JSON line with the mismatch count.  usage: python tests/stress_jpeg.py [cases] [seed]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import np_jpeg as J  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector  # noqa: E402


def content(rng, h, w):
    if rng.random() < 0.4:
        return (rng.random((h, w)) * 256).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    a, b = rng.uniform(3, 40, 2)
    base = 128 + 70 * np.sin(xx / a) * np.cos(yy / b) + 50 * ((xx // int(a + 2) + yy // int(b + 2)) % 2)
    return np.clip(base + rng.normal(0, rng.uniform(0, 20), (h, w)), 0, 255).astype(np.uint8)


def stream(rng, h, w):
    samp = str(rng.choice(list(J.SAMPLINGS)))
    kind = int(rng.integers(0, 4))
    kw = dict(sampling=samp, quality=int(rng.integers(1, 101)), dht=rng.random() > 0.2, q16=rng.random() < 0.2)
    if kind == 1:
        kw["restart_interval"] = int(rng.integers(1, 10))
    elif kind == 2:
        kw.update(restart_interval=int(rng.integers(1, 3)), restart_rows=True)
    if kw["dht"] and rng.random() < 0.3:
        kw["tables"] = {(c, s): J.shuffled_table(c, s, rng) for c in (0, 1) for s in (0, 1)}
    return J.encode(content(rng, h, w), **kw)


def run(cases, seed):
    rng = np.random.default_rng(seed)
    bad = frames = 0
    for c in range(cases):
        w, h = int(rng.integers(16, 401)), int(rng.integers(16, 401))
        n = int(rng.integers(1, 5))
        streams = [stream(rng, h, w) for _ in range(n)]
        det = AprilTagDetector(w, h, max_batch=n)
        got, st = det.decode_jpeg(streams, return_status=True)
        det.close()
        for i, b in enumerate(streams):
            frames += 1
            want, wst = J.decode_luma(b)
            if st[i] != wst or not np.array_equal(got[i], want):
                bad += 1
                print("MISMATCH case", c, "frame", i, (w, h), "status", st[i], wst, flush=True)
    print(json.dumps({"stress": "jpeg", "cases": cases, "seed": seed, "frames": frames, "mismatching": bad}), flush=True)
    return bad


if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    sys.exit(1 if run(cases, seed) else 0)
