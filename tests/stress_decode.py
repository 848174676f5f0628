"""Randomised parity stress of the decode stage against the CPU oracle, detection for detection (test infrastructure: imports
oracle/), through ck_decode_quads_batch.  A case draws: one or two families (built-in, tests/family_gen.py's geometries, tag36h11's
and full64's layouts grown to 600..2200 codes) and with them the code count; 1..3 frames on a handle of up to two more; per frame
0..quad_cap tags, turned by any angle, mildly tilted, 14..70 pixels, anywhere including over the frame's sides; 0..max_hamming + 1
flipped bits; decode_sharpening 0, 0.25, 0.5 or 1; max_hamming 0..3; the quads are the drawn corners, some of them with their corners
cycled, moved by a fraction of a pixel, repeated, or with the other border sense.  Every frame's detection bytes, count and status
must equal the oracle's.  No case is left out: every drawn case is within the handle's capacities by construction (quads <=
max_quads_per_frame; candidates <= quads x families).
usage: python tests/stress_decode.py [cases] [seed]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
import numpy as np
import pyoracle
import decode_cases as dc
import np_tag_render as tr

FAMILIES = ["tag36h11", "tag16h5", "std41n", "std41r", "circ21r", "std52r", "full64", "full64w", "t36n600", "t36n769", "t36n1537", "t36n2200",
            "f64n900", "f64n1600", "t36sym"]


def draw(rng, c):
    w, h = int(rng.integers(96, 421)), int(rng.integers(80, 401))
    n = int(rng.integers(1, 4))
    fams = [str(f) for f in rng.choice(FAMILIES, int(rng.integers(1, 3)), replace=False)]
    mh = int(rng.integers(0, 4))
    qcap = int(rng.choice([4, 16, 64]))
    settings = {"families": fams, "max_hamming": mh, "decode_sharpening": float(rng.choice([0.0, 0.25, 0.5, 1.0])), "max_quads_per_frame": qcap}
    frames, quads = [], []
    for i in range(n):
        k = int(rng.integers(0, qcap + 1)) if rng.random() < 0.8 else qcap
        tags, qs = [], []
        for _ in range(min(k, 12)):
            name = fams[int(rng.integers(0, len(fams)))]
            p = dc.fam(name).contents
            side = float(rng.uniform(14, 70))
            corners = tr.pose(rng.uniform(-0.2 * side, w + 0.2 * side), rng.uniform(-0.2 * side, h + 0.2 * side), side, rng.uniform(0, 360),
                              tuple(rng.uniform(-0.04, 0.04, 2)))
            flips = tuple(int(b) for b in rng.choice(p.nbits, int(rng.integers(0, mh + 2)), replace=False))
            tags.append((name, int(rng.integers(0, p.ncodes)), corners, flips))
            qs.append(dc.quad(corners, p.reversed_border))
        frame = dc.draw(w, h, tags, seed=int(rng.integers(1, 10000)), noise=float(rng.uniform(0, 3)))
        while len(qs) < k:   # variations of the drawn quads, or quads over nothing
            if tags and rng.random() < 0.8:
                name, _, corners, _ = tags[int(rng.integers(0, len(tags)))]
                rev = dc.fam(name).contents.reversed_border
                kind = int(rng.integers(0, 4))
                if kind == 0: qs.append(dc.quad(dc.cycled(corners, int(rng.integers(1, 4))), rev))
                elif kind == 1: qs.append(dc.quad(corners + rng.uniform(-0.7, 0.7, (4, 2)), rev))
                elif kind == 2: qs.append(dc.quad(corners, rev))
                else: qs.append(dc.quad(corners, 1 - rev))
            else:
                qs.append(dc.quad(rng.integers(-8, max(w, h) // 4, (4, 2)) * 4.0, int(rng.integers(0, 2))))
        order = rng.permutation(len(qs))
        frames.append(frame); quads.append([qs[j] for j in order])
    info = {"case": c, "w": w, "h": h, "n": n, "settings": settings, "quads": [len(q) for q in quads]}
    case = {"frames": np.stack(frames), "quads": quads, "settings": settings, "truth": [{} for _ in quads],
            "cap": int(rng.choice([4, 64, 256])), "max_batch": n + c % 3}
    return info, case


def run(cases, seed):
    rng = np.random.default_rng(seed)
    bad = total = 0
    for c in range(cases):
        info, case = draw(rng, c)
        if os.environ.get("STRESS_LOG"):
            with open(os.environ["STRESS_LOG"], "a") as lf:
                lf.write(json.dumps(info) + "\n")
        diffs, _, found = dc.run_case(dc.detector, pyoracle, case)
        total += found
        if diffs:
            bad += 1
            print(json.dumps(dict(info, diffs=diffs[:6])))
    print(json.dumps({"cases": cases, "left_out": 0, "oracle_detections": total, "mismatching_cases": bad}))
    if total < cases:   # (a run whose drawn tags decode nowhere compares empty lists: about 3 to 5 detections per case are usual)
        print(json.dumps({"error": "fewer detections than cases: the drawing is broken"}))
        return bad + 1
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 30, int(sys.argv[2]) if len(sys.argv) > 2 else 1) else 0)
