"""Randomised stress of the per-tag pose (test infrastructure): random poses (0.3..12 m, tilt up to 85 degrees), corner noise,
cameras, OpenCV-5 distortion on half the cases, tag sizes and families (four in one handle), n_iters 1..200.  Every case goes
through ck_estimate_tag_poses on the GPU and through tests/np_tag_pose.py; a record that differs beyond the tolerances of
tests/tag_pose_util.py (borderline has_alt cases and error ties excepted, as there) is a mismatch.  Prints the mismatch count.
usage: python tests/stress_tag_pose.py [cases] [seed]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import tag_pose_util as U  # noqa: E402
from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector, _raw_detections, tag_pose_params  # noqa: E402


def run(cases, seed):
    rng = np.random.default_rng(seed)
    det = AprilTagDetector(64, 64, max_batch=1, families=("tag36h11", "tag16h5", "tag36h11", "tag16h5"))
    bad, stats, done = [], {}, 0
    while done < cases:
        k = min(200, cases - done)
        f = rng.uniform(300, 2000)
        dist = tuple(rng.uniform(-0.05, 0.05, 5) * [1, 0.2, 0.02, 0.02, 0.1]) if rng.random() < 0.5 else (0.0,) * 5
        cam = (f, f * rng.uniform(0.98, 1.02), rng.uniform(200, 1000), rng.uniform(150, 700)) + dist
        sizes = list(rng.uniform(0.02, 0.5, 4))
        n_iters = int(rng.choice([1, 7, 50, 50, 50, 200]))
        noise = float(rng.choice([0.0, 0.1, 0.5, 2.0]))
        recs = []
        for i in range(k):
            fam = int(rng.integers(0, 4))
            R, t = U.random_pose(rng, 0.3, 12.0, 85.0)
            c = U.project(R, t, sizes[fam] / 2, cam[:4] + (0.0,) * 5) + rng.normal(0, noise, (4, 2))
            d = A.Detection()
            d.id, d.family = i, fam
            for q in range(4):
                d.p[q][0], d.p[q][1] = c[q]
            recs.append(d)
        arr, n = _raw_detections(recs)
        pp = tag_pose_params(*cam[:4], tagsize=sizes, distortion=cam[4:], n_iters=n_iters)
        gpu = U.records_of(det.estimate_tag_poses(arr, pp, raw=True))
        ref, infos = U.np_poses(arr, cam, sizes, n_iters)
        b = U.compare(gpu, ref, infos, stats)
        bad += [(done + i, what) for i, what, *_ in b]
        done += k
    print(json.dumps({"cases": cases, "seed": seed, "mismatches": len(bad), "first": [list(map(str, x)) for x in bad[:5]],
                      "max_dR": stats["dR"], "max_dt": stats["dt"], "max_derr": stats["derr"], "with_alt": stats["alts"],
                      "borderline": stats["borderline"], "ties": stats["ties"]}))
    return len(bad)


if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    sys.exit(1 if run(cases, seed) else 0)
