"""Child of tests/test_gpu_span_alignment.py: runs the frames of one .npz file (per handle NAME: frames f_NAME, the oracle's sorted
quads q_NAME_i of frame i) through AprilTagDetector.quads on whatever build of the library the environment names, once per base with
CK_EXT_BASE set to it (the diagnostics build reads it per call), compares bit for bit and prints the first mismatching (base, handle,
frame), the number of mismatches, a hash of everything the device returned and the seconds the calls took.
usage: python tests/span_alignment_child.py cases.npz NAME[,NAME...] BASES     (BASES: comma-separated numbers and ranges lo:hi)"""
import hashlib
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
import numpy as np
import pyoracle
import quad_cases as qc


def parse_bases(spec):
    out = []
    for part in spec.split(","):
        lo, _, hi = part.partition(":")
        out += list(range(int(lo), int(hi))) if hi else [int(lo)]
    return out


def run(path, names, bases):
    z = np.load(path)
    hh, bad, calls = hashlib.sha256(), [], 0
    dets = {}
    for name in names:
        n, h, w = z["f_" + name].shape
        dets[name] = (qc.detector(w, h, n, {}), z["f_" + name], [z["q_%s_%d" % (name, i)] for i in range(n)])
    t0 = time.time()
    for base in bases:
        os.environ["CK_EXT_BASE"] = str(base)
        for name in names:
            det, frames, want = dets[name]
            got = det.quads(frames)
            calls += 1
            for i, w in enumerate(want):
                a = qc.sort_quads(pyoracle.quads_to_np(got[i]))
                hh.update(np.int64(len(a)).tobytes()); hh.update(np.ascontiguousarray(a, np.float64).tobytes())
                if a.shape != w.shape or a.tobytes() != w.tobytes():
                    bad.append((base, name, i, len(a), len(w)))
    seconds = time.time() - t0
    for det, _, _ in dets.values():
        det.close()
    for b in bad[:16]:
        print("MISMATCH base %d handle %s frame %d: %d quads, the oracle %d" % b)
    print("CALLS", calls)
    print("MISMATCHES", len(bad))
    print("HASH", hh.hexdigest())
    print("SECONDS %.2f" % seconds)
    return len(bad)


if __name__ == "__main__":
    sys.exit(1 if run(sys.argv[1], sys.argv[2].split(","), parse_bases(sys.argv[3])) else 0)
