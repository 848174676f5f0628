"""Randomised parity stress of quad_sigma (test infrastructure: imports oracle/): random sizes 16..700, sigma uniform in [-8, 8],
quad_decimate 1 or 2, random noise levels.  Per frame the quad image must equal the numpy restatement (tests/quad_filter_ref.py),
threshold / segmentation the oracle's on it, and the detections the oracle's pipeline on it (refinement and decode on Q at
quad_decimate 1, on the frame at 2).  Prints mismatch counts per stage.  usage: python tests/stress_quad_sigma.py [cases] [seed]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pyoracle
import quad_filter_ref as R
from chalkydri_amd import _abi as A
from chalkydri_amd import default_config, synth
from chalkydri_amd.detector import AprilTagDetector


def oracle_dets(frame, q, cfg, dec):
    if dec == 1:
        return pyoracle.detect(q, cfg)[0]
    th = pyoracle.threshold(q)
    lab, sz = pyoracle.segment(th)
    cl, pts, _ = pyoracle.clusters(th, lab, sz)
    quads, _ = pyoracle.fit_quads(frame, cfg, cl, pts, quad_img=q)
    h, w = frame.shape
    qa = (A.Quad * max(len(quads), 1))(*quads)
    dets = (A.Detection * 256)()
    nd = C.c_int(0)
    pyoracle.lib().ora_decode_quads(C.c_void_p(frame.ctypes.data), w, h, w, C.byref(cfg), qa, len(quads), dets, 256, C.byref(nd))
    return pyoracle.dets_to_list(dets, nd.value)


def run(cases, seed):
    rng = np.random.default_rng(seed)
    bad = {"quad_image": 0, "threshold": 0, "segment": 0, "detections": 0}
    frames_seen = 0
    for c in range(cases):
        dec = int(rng.integers(1, 3))
        w, h = int(rng.integers(16, 701)), int(rng.integers(16, 701))
        n = int(rng.integers(1, 4))
        sigma = float(np.float32(rng.uniform(-8.0, 8.0)))
        noise = int(rng.choice([0, 2, 6, 16]))
        if min(w, h) >= 120:
            frames = synth.render_batch(7000 + c, n, w, h, int(rng.integers(0, 5)), noise_amp=noise, min_side=24,
                                        max_side=max(24, min(w, h) // 3))[0]
        else:
            frames = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
        det = AprilTagDetector(w, h, max_batch=n, quad_decimate=dec, quad_sigma=sigma)
        cfg = default_config(w, h, quad_decimate=dec)
        qimg = det.quad_image(frames)
        th = det.threshold(frames)
        labels, sizes = det.segment(frames)
        dets = det.detect_batch(frames, cap=256)
        det.close()
        for i in range(n):
            frames_seen += 1
            q = R.quad_image(frames[i], sigma, dec)
            oth = pyoracle.threshold(q)
            olab, osz = pyoracle.segment(oth)
            want = oracle_dets(frames[i], q, cfg, dec)
            got = [(d.id(), d.hamming(), d.corners().tobytes()) for d in dets[i]]
            exp = [(d["id"], d["hamming"], d["p"].tobytes()) for d in want]
            res = {"quad_image": np.array_equal(qimg[i], q), "threshold": np.array_equal(th[i], oth),
                   "segment": np.array_equal(labels[i], olab) and np.array_equal(sizes[i], osz), "detections": got == exp}
            for k, ok in res.items():
                if not ok:
                    bad[k] += 1
            if not all(res.values()):
                print(json.dumps({"case": c, "frame": i, "w": w, "h": h, "dec": dec, "sigma": sigma, "noise": noise,
                                  "mismatch": [k for k, ok in res.items() if not ok]}))
    print(json.dumps({"cases": cases, "frames": frames_seen, "seed": seed, "mismatching_frames": bad}))
    return sum(bad.values())


if __name__ == "__main__":
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 60, int(sys.argv[2]) if len(sys.argv) > 2 else 1) else 0)
