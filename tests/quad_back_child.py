"""Child of tests/test_gpu_quad_back.py: runs the cases of one .npz file (frames f_NAME, settings s_NAME as a JSON string, frame index
u_NAME, the oracle's quads q_NAME_i) through AprilTagDetector.quads on whatever build of the library the environment names, compares
bit for bit and prints the mismatching cases and a hash of everything the device returned.
usage: python tests/quad_back_child.py cases.npz"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
import numpy as np
import pyoracle
import quad_cases as qc


def run_case(z, name, hh=None):
    """Frames of case `name` that differ from the oracle: (frame, device quads, oracle quads)."""
    frames, settings = z["f_" + name], json.loads(str(z["s_" + name]))
    n, h, w = frames.shape
    det = qc.detector(w, h, n, settings)
    got = det.quads(frames)
    det.close()
    bad = []
    for i in range(n):
        a = qc.sort_quads(pyoracle.quads_to_np(got[i]))
        if hh is not None:
            hh.update(np.int64(len(a)).tobytes()); hh.update(np.ascontiguousarray(a, np.float64).tobytes())
        want = z["q_%s_%d" % (name, int(z["u_" + name][i]))]
        if a.shape != want.shape or a.tobytes() != want.tobytes():
            bad.append((i, len(a), len(want)))
    return bad


def run(path):
    z = np.load(path)
    bad, hh = 0, hashlib.sha256()
    for name in sorted(k[2:] for k in z.files if k.startswith("f_")):
        frames_bad = run_case(z, name, hh)
        if frames_bad:
            bad += 1
            print("MISMATCH", name, json.dumps(frames_bad[:8]))
    print("MISMATCHING_CASES", bad)
    print("HASH", hh.hexdigest())
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(sys.argv[1]) else 0)
