"""Child of tests/test_gpu_seq_front.py: runs the cases of one .npz file (frames f_NAME, the oracle's quads q_NAME_i) through
AprilTagDetector.quads on whatever build of the library the environment names, compares bit for bit and prints the number of
mismatching frames and a hash of everything the device returned.  usage: python tests/seq_front_child.py cases.npz"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np
import pyoracle
from chalkydri_amd.detector import AprilTagDetector


def run(path):
    z = np.load(path)
    bad, hh = 0, hashlib.sha256()
    for name in sorted(k[2:] for k in z.files if k.startswith("f_")):
        frames = z["f_" + name]
        n, h, w = frames.shape
        det = AprilTagDetector(w, h, max_batch=n)
        got = det.quads(frames)
        _, status = det.detect_batch(frames, cap=64, return_status=True)
        hh.update(np.asarray(status, np.uint32).tobytes())
        for i in range(n):
            a = pyoracle.quads_to_np(got[i])
            a = a[np.lexsort((a[:, 10], a[:, 9]))] if len(a) else a
            hh.update(np.int64(len(a)).tobytes()); hh.update(np.ascontiguousarray(a, np.float64).tobytes())
            want = z["q_%s_%d" % (name, int(z["u_" + name][i]))]
            if a.shape != want.shape or not np.array_equal(a, want):
                bad += 1
                print("MISMATCH case", name, "frame", i, "have", len(a), "want", len(want))
        det.close()
    print("MISMATCHING_FRAMES", bad)
    print("HASH", hh.hexdigest())
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(sys.argv[1]) else 0)
