"""Randomised parity stress of the whole detector against the CPU oracle on the test families of tests/family_gen.py (test
infrastructure: imports oracle/): each case draws a set of up to four families (reversed and normal borders, odd bit counts,
bits outside the border, 64-bit words, tag36h11 among them), a geometry, decimation, detector settings and max_hamming, draws
frames with tests/np_tag_render.py (some tags with inverted bits) and compares detections bit for bit (id, hamming, family,
margin, centre, corners) and the status word.  usage: python tests/stress_families.py [cases] [seed]
python tests/stress_families.py --quads: the quad parity cases of QUAD_CASES only (reversed-only and mixed configurations), for a child
process that forces a fit path (CK_FIT_FLAT=2 of the diagnostics build: the split fit)."""
import os, sys, json
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
import numpy as np
import pyoracle
import family_gen as fg
import np_tag_render
from chalkydri_amd import default_config, family
from chalkydri_amd.detector import AprilTagDetector

NAMES = ["tag36h11"] + list(fg.MATRIX)


def run(cases, seed):
    rng = np.random.default_rng(seed)
    bad = 0
    for c in range(cases):
        k = int(rng.integers(1, 5))
        names = [NAMES[i] for i in rng.choice(len(NAMES), k, replace=False)]
        fams = tuple(family(n) if n.startswith("tag") else fg.make(n) for n in names)
        dec = int(rng.choice([1, 1, 2]))
        w, h = int(rng.integers(200, 900)), int(rng.integers(160, 700))
        cols, rows = int(rng.integers(1, 5)), int(rng.integers(1, 4))
        n = int(rng.integers(1, 4))
        bits = int(rng.choice([0, 1, 2, 2]))       # every family keeps min_hamming > 2 bits + 1 (circ21r has 6)
        flips = int(rng.choice([0, 0, 1, 2, 3]))
        noise = float(rng.choice([0.0, 1.5, 4.0]))
        side = (max(16.0, min(w / cols, h / rows) * 0.2), max(20.0, min(w / cols, h / rows) * 0.5))
        settings = {}
        if rng.random() < 0.3: settings["refine_edges"] = 0
        if rng.random() < 0.2: settings["max_nmaxima"] = int(rng.integers(4, 13))
        if rng.random() < 0.2: settings["min_cluster_pixels"] = int(rng.choice([5, 24, 50]))
        if rng.random() < 0.2: settings["decode_sharpening"] = float(rng.choice([0.0, 0.25, 1.0]))
        if os.environ.get("STRESS_LOG"):
            with open(os.environ["STRESS_LOG"], "a") as lf:
                lf.write(json.dumps({"case": c, "w": w, "h": h, "n": n, "fams": names, "dec": dec, "bits": bits, "flips": flips,
                                     "settings": settings}) + "\n")
        frames = np.stack([np_tag_render.scene(fams, 1000 * c + i + seed, w=w, h=h, cols=cols, rows=rows, side=side, noise=noise,
                                               flips=flips)[0] for i in range(n)])
        det = AprilTagDetector(w, h, max_batch=n, families=fams, quad_decimate=dec, bits_corrected=bits, **settings)
        got, status = det.detect_batch(frames, cap=256, return_status=True)
        cfg = default_config(w, h, families=fams, quad_decimate=dec, max_hamming=bits, **settings)
        for i in range(n):
            want, st = pyoracle.detect(frames[i], cfg)
            ok = status[i] == st and len(got[i]) == len(want)
            if ok:
                for a, b in zip(got[i], want):
                    ok = ok and (a.id(), a.hamming(), a.family()) == (b["id"], b["hamming"], b["family"]) and \
                        np.float32(a.decision_margin()) == np.float32(b["margin"]) and np.array_equal(a.center(), b["c"]) and np.array_equal(a.corners(), b["p"])
            if not ok:
                bad += 1
                print(json.dumps({"case": c, "frame": i, "w": w, "h": h, "dec": dec, "fams": names, "got": len(got[i]), "want": len(want),
                                  "status": [int(status[i]), int(st)]}))
        det.close()
    print(json.dumps({"cases": cases, "mismatching_frames": bad}))
    return bad


# (family names, quad_decimate): a reversed-only configuration (every quad has reversed_border 1) and a mixed one
QUAD_CASES = [(names, dec) for names in (("std41r", "std52r"), ("tag36h11", "std41r", "full64", "circ21r")) for dec in (1, 2)]


def _quads_sorted(quads):
    a = pyoracle.quads_to_np(quads)
    return a[np.lexsort((a[:, 10], a[:, 9]))] if len(a) else a


def quad_parity(names, dec, w=801, h=601, n=2):
    """ck_quads_batch against ora_fit_quads on frames of the named families.  Returns (mismatching frames, set of reversed_border
    values seen, fewest quads in a frame)."""
    fams = tuple(family(x) if x.startswith("tag") else fg.make(x) for x in names)
    frames = np.stack([np_tag_render.scene(list(fams), 90 + dec + i, w=w, h=h, cols=4, rows=3)[0] for i in range(n)])
    det = AprilTagDetector(w, h, max_batch=n, families=fams, quad_decimate=dec)
    got = det.quads(frames)
    det.close()
    cfg = default_config(w, h, families=fams, quad_decimate=dec)
    bad, flags, fewest = 0, set(), 1 << 30
    for i in range(n):
        want, have = _quads_sorted(pyoracle.quads(frames[i], cfg)), _quads_sorted(got[i])
        if want.shape != have.shape or not np.array_equal(want, have):
            bad += 1
            print(json.dumps({"quads": list(names), "dec": dec, "frame": i, "want": len(want), "have": len(have)}))
        flags |= set(int(v) for v in have[:, 8]) if len(have) else set()
        fewest = min(fewest, len(have))
    return bad, flags, fewest


def run_quads():
    bad = 0
    for names, dec in QUAD_CASES:
        b, flags, fewest = quad_parity(names, dec)
        reversed_only = all(not x.startswith("tag") and fg.MATRIX[x][3] for x in names)
        if flags != ({1} if reversed_only else {0, 1}) or fewest < 12:
            b += 1
            print(json.dumps({"quads": list(names), "dec": dec, "reversed_border_values": sorted(flags), "fewest_quads": fewest}))
        bad += b
    print(json.dumps({"quad_cases": len(QUAD_CASES), "quad_mismatching_frames": bad}))
    return bad


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--quads":
        sys.exit(1 if run_quads() else 0)
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 60, int(sys.argv[2]) if len(sys.argv) > 2 else 1) else 0)
