"""Child of tests/test_gpu_emit_rows.py: every frame of tests/emit_row_cases.py through AprilTagDetector.clusters on whatever build of
the library the environment names (the diagnostics build with CK_EMIT_TWINS=0 and / or CK_POISON=1), checked point for point
against the oracle.  Prints one line: EMIT_ROWS_CHILD <frames checked> <points returned>."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
import numpy as np
import cluster_cases as cc
import emit_row_cases as ec


def check_batch(oracle, w, h, min_component_px, named, wants=None):
    """one call of clusters() over the frames of {name: frame}, every frame against the oracle's clusters; returns the points returned"""
    from chalkydri_amd.detector import AprilTagDetector
    names = list(named)
    if wants is None:
        wants = [cc.oracle_clusters(oracle, named[n], min_component_px) for n in names]
    det = AprilTagDetector(w, h, max_batch=len(names), min_component_px=min_component_px)
    ccap, pcap = cc.caps_for(wants)
    got = det.clusters(np.stack([named[n] for n in names]), cluster_cap=ccap, point_cap=pcap)
    for i, n in enumerate(names):
        cc.check_frame(got[i], wants[i], f"{w}x{h} min_component_px={min_component_px} {n}")
    det.close()
    return sum(len(g[1]) for g in got)


def run():
    import pyoracle
    frames = points = 0
    for w, h in ec.SIZES:
        named = ec.frames(w, h)
        for mcp in ec.MIN_COMPONENT:
            points += check_batch(pyoracle, w, h, mcp, named)
            frames += len(named)
    w, h, mcp, named = ec.rim_noise()
    points += check_batch(pyoracle, w, h, mcp, named)
    frames += len(named)
    print("EMIT_ROWS_CHILD", frames, points)


if __name__ == "__main__":
    run()
