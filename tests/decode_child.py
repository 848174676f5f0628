"""Child of tests/test_gpu_decode.py: every case of tests/decode_cases.py through AprilTagDetector.decode_quads on whatever build of the
library and whatever allocation fill the environment names, the quad lists in the order of seed `shuffle`; prints the mismatching
cases and a hash of everything the device returned.
usage: python tests/decode_child.py [shuffle seed]"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
import pyoracle
import decode_cases as dc


def run(shuffle):
    bad, hh = 0, hashlib.sha256()
    for name in dc.NAMES:
        diffs, blob, _ = dc.run_case(dc.detector, pyoracle, name, shuffle=shuffle)
        hh.update(blob)
        if diffs:
            bad += 1
            print("MISMATCH", json.dumps(diffs[:8]))
    print("MISMATCHING_CASES", bad)
    print("HASH", hh.hexdigest())
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else None) else 0)
