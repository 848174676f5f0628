"""Randomised parity stress of the gradient-cluster stage against the CPU oracle (test infrastructure: imports oracle/): random
geometries (ragged included), two kinds of content side by side, 1..6 frames, quad_decimate 1 or 2, min_component_px from
{1, 5, 25, 200, 40000}, min_cluster_pixels from {5, 24, 50}; every cluster inside k_scan's gates must come back with the oracle's
key and the oracle's points (sorted: the order inside a cluster is not defined on the device), the records tiling the point array.
A case in which a frame has more distinct component pairs than the handle's table has entries (2 * max(1024, qw * qh / 32), rounded
up to a power of two), more kept clusters than its cluster list (max(1024, qw * qh / 32)), more runs than its run list or more
than 512 pairs in one emit tile is left out and counted; more than a tenth of the cases left out fails the run.
usage: python tests/stress_clusters.py [cases] [seed] [--oracle-only]   (--oracle-only: no GPU, prints which cases would be left out)"""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pyoracle
import cluster_cases as cc

KINDS = ["synth", "noise", "flat", "stripes", "blobs", "spiral", "checker1", "vstripes1"]
# the one-pixel kinds are drawn less often: at min_component_px = 1 a checkerboard is a component pair per dark pixel, far more than any
# handle's table, and such a case is only ever left out
KIND_P = [0.13, 0.14, 0.13, 0.13, 0.14, 0.13, 0.10, 0.10]


def _pow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


def draw(rng, c):
    """Case c: its settings, its frames, the oracle's clusters per frame, and why it is left out (or None)."""
    w = int(rng.integers(40, 700)); h = int(rng.integers(40, 500))
    if rng.random() < 0.3: w = (w // 4) * 4
    n = int(rng.integers(1, 7))
    dec = int(rng.choice([1, 2]))
    mcp = int(rng.choice([1, 5, 25, 200, 40000]))
    mcl = int(rng.choice([5, 24, 50]))
    ka, kb = rng.choice(KINDS, 2, p=KIND_P)
    sa, sb = int(rng.integers(1, 1000)), int(rng.integers(1, 1000))
    x0, y0 = int(rng.integers(0, w // 2)), int(rng.integers(0, h // 2))
    frames = cc.side_by_side(cc._seg_frames(str(ka), w, h, n, sa), cc._seg_frames(str(kb), w, h, n, sb), x0, y0)
    info = {"case": c, "w": w, "h": h, "n": n, "dec": dec, "min_component_px": mcp, "min_cluster_pixels": mcl, "kinds": [str(ka), str(kb)],
            "seeds": [sa, sb], "x0": x0, "y0": y0}
    qw, qh = w // dec, h // dec
    ccap = max(1024, qw * qh // 32)
    table = _pow2(2 * ccap)
    wants, left = [], None
    for i in range(n):
        th, lab, sz = cc.oracle_stages(pyoracle, frames[i], dec)
        cl, pts, ov = pyoracle.clusters(th, lab, sz, mcp)
        lo, hi = cc.gate(qw, qh, mcl)
        want = cc.cluster_dict(cl, pts, lo, hi)
        if len(cl) > table: left = left or "pairs %d > table %d" % (len(cl), table)
        if len(want) > ccap: left = left or "kept %d > cluster list %d" % (len(want), ccap)
        # the handle's two other capacities of this stage (both documented; neither was met by a case that the two rules above keep):
        # the run list (4 x the cluster list) and the 512 pairs of one emit tile (include/chalkydri_hip.h at CK_FRAME_CLUSTERS_OVERFLOW)
        st = cc.emit_stats(th, lab, sz, mcp, mcl)
        if st.runs > 4 * ccap: left = left or "runs %d > run list %d" % (st.runs, 4 * ccap)
        if int(st.pairs_per_tile.max()) > 512: left = left or "pairs in one emit tile %d > 512" % int(st.pairs_per_tile.max())
        wants.append(want)
    return info, frames, wants, left


def run(cases, seed, oracle_only=False):
    rng = np.random.default_rng(seed)
    bad = left_out = 0
    for c in range(cases):
        info, frames, wants, left = draw(rng, c)
        if os.environ.get("STRESS_LOG"):
            with open(os.environ["STRESS_LOG"], "a") as lf:
                lf.write(json.dumps(dict(info, left_out=left)) + "\n")
        if left:
            left_out += 1
            print(json.dumps(dict(info, left_out=left)))
            continue
        if oracle_only:
            continue
        from chalkydri_amd.detector import AprilTagDetector
        extra = int(info["case"] % 3)   # the handle is sized for more frames than the call brings
        det = AprilTagDetector(info["w"], info["h"], max_batch=info["n"] + extra, quad_decimate=info["dec"], min_component_px=info["min_component_px"],
                               min_cluster_pixels=info["min_cluster_pixels"])
        ccap, pcap = cc.caps_for(wants)
        try:
            got = det.clusters(frames, cluster_cap=ccap, point_cap=pcap)
            for i in range(info["n"]):
                try:
                    cc.check_frame(got[i], wants[i], "frame %d" % i)
                except AssertionError as e:
                    bad += 1
                    print(json.dumps(dict(info, frame=i, error=str(e))))
        except Exception as e:   # (ChalkydriError: a result that does not fit the capacities taken from the oracle's counts)
            bad += info["n"]
            print(json.dumps(dict(info, error=str(e))))
        det.close()
    print(json.dumps({"cases": cases, "left_out": left_out, "mismatching_frames": bad}))
    if left_out * 10 > cases:
        print(json.dumps({"error": "more than a tenth of the cases left out"}))
        return bad + 1
    return bad


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    sys.exit(1 if run(int(args[0]) if len(args) > 0 else 60, int(args[1]) if len(args) > 1 else 1, "--oracle-only" in sys.argv) else 0)
