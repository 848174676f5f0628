"""Child of tests/test_gpu_twin_points.py: two random 320 x 200 frames (noise; rendered tags under noise) through
AprilTagDetector.clusters and detect_batch on whatever build of the library the environment names, compared with the oracle.
Prints one line: TWIN_CHILD <points returned> <mismatching frames> <hash of everything the device returned>."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
import numpy as np
import pyoracle
import cluster_cases as cc
from chalkydri_amd import default_config
from chalkydri_amd.detector import AprilTagDetector

W, H = 320, 200


def run():
    frames = np.stack([cc.frame("noise", W, H, 41), cc.frame("tags", W, H, 42)])
    wants = [cc.oracle_clusters(pyoracle, f) for f in frames]
    det = AprilTagDetector(W, H, max_batch=2)
    ccap, pcap = cc.caps_for(wants)
    got = det.clusters(frames, cluster_cap=ccap, point_cap=pcap)
    dets, status = det.detect_batch(frames, cap=64, return_status=True)
    cfg = default_config(W, H)
    bad, points, hh = 0, 0, hashlib.sha256()
    hh.update(np.asarray(status, np.uint32).tobytes())
    for i in range(2):
        have = cc.cluster_dict(*got[i])
        points += len(got[i][1])
        for k in sorted(have):
            hh.update(np.asarray(k, np.int64).tobytes()); hh.update(have[k].tobytes())
        want_dets, st = pyoracle.detect(frames[i], cfg)
        mine = [(d.id(), d.hamming(), d.corners().tobytes(), d.center().tobytes()) for d in dets[i]]
        for d in mine:
            hh.update(repr(d).encode())
        ok = set(have) == set(wants[i]) and all(np.array_equal(have[k], wants[i][k]) for k in have) and len(have) == len(got[i][0])
        ok = ok and status[i] == st and mine == [(d["id"], d["hamming"], d["p"].tobytes(), d["c"].tobytes()) for d in want_dets]
        bad += 0 if ok else 1
    det.close()
    print("TWIN_CHILD", points, bad, hh.hexdigest())
    return bad


if __name__ == "__main__":
    sys.exit(1 if run() else 0)
