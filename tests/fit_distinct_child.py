"""Child of tests/test_gpu_fit_distinct.py: runs the cases of one .npz file (tests/fit_distinct_cases.py: save_cases) through
AprilTagDetector.quads and detect_batch on whatever build of the library the environment names, with whatever knobs it sets, compares
quads, detections and status words bit for bit with the oracle's and prints the number of mismatching frames and a hash of everything
the device returned.  usage: python tests/fit_distinct_child.py cases.npz"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
import numpy as np
import pyoracle
from chalkydri_amd.detector import AprilTagDetector


def det_rows(ds):
    return np.asarray([[d.family(), d.id(), d.hamming(), np.float32(d.decision_margin()), *d.center(), *np.asarray(d.corners()).reshape(-1)] for d in ds],
                      np.float64).reshape(-1, 14)


def run(path):
    z = np.load(path)
    bad, hh = 0, hashlib.sha256()
    for name in sorted(k[2:] for k in z.files if k.startswith("f_")):
        frames = z["f_" + name]
        settings = json.loads(bytes(z["s_" + name]).decode())
        n, h, w = frames.shape
        det = AprilTagDetector(w, h, max_batch=n, **settings)
        got = det.quads(frames)
        dets, status = det.detect_batch(frames, cap=64, return_status=True)
        det.close()
        status = np.asarray(status, np.uint32)
        hh.update(status.tobytes())
        for i in range(n):
            q = pyoracle.quads_to_np(got[i])
            q = q[np.lexsort((q[:, 10], q[:, 9]))] if len(q) else q
            d = det_rows(dets[i])
            for a in (q, d):
                hh.update(np.int64(len(a)).tobytes()); hh.update(np.ascontiguousarray(a, np.float64).tobytes())
            wq, wd = z[f"q_{name}_{i}"], z[f"d_{name}_{i}"]
            same = q.shape == wq.shape and np.array_equal(q, wq) and d.shape == wd.shape and np.array_equal(d, wd) and status[i] == z["st_" + name][i]
            if not same:
                bad += 1
                print("MISMATCH case", name, "frame", i, "quads", len(q), "want", len(wq), "detections", len(d), "want", len(wd), "status",
                      int(status[i]), "want", int(z["st_" + name][i]))
    print("MISMATCHING_FRAMES", bad)
    print("HASH", hh.hexdigest())
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(sys.argv[1]) else 0)
