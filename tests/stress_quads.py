"""Randomised parity stress of the quad fit against the CPU oracle, quad for quad (test infrastructure: imports oracle/): random
geometries (ragged included), 1..4 frames, quad_decimate 1 or 2, two kinds of content side by side out of rendered tag scenes with
noise, the sheets of small squares and discs and the symmetric blobs of tests/quad_cases.py, and the quad-fit settings of
tests/stress_detect.py (max_nmaxima 4..12, max_line_fit_mse, cos_critical_rad, refine_edges, min_component_px, min_cluster_pixels).
Every frame's quads, sorted by (rep0, rep1), must equal the oracle's byte for byte: a wrong quad shows here whether it decodes or not.
A case in which a frame has more component pairs or kept clusters than the handle's lists hold (tests/stress_clusters.py has the
rule) is left out and counted; more than a tenth of the cases left out fails the run.
usage: python tests/stress_quads.py [cases] [seed]"""
import os, sys, json
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
import numpy as np
import pyoracle
import cluster_cases as cc
import quad_cases as qc

KINDS = ["tags", "squares", "discs", "blobs"]


def content(kind, w, h, n, seed):
    """n frames [h][w] of one kind, every frame from its own seed"""
    if kind == "tags":
        from chalkydri_amd import synth
        kw = {"noise_amp": 1 + seed % 4}
        if min(w, h) < 300:
            kw.update(min_side=24, max_side=max(24, min(w, h) // 3))
        return synth.render_batch(40 + seed, n, w, h, 1 + seed % 5, **kw)[0]
    out = np.full((n, h, w), qc.BRIGHT, np.uint8)
    for i in range(n):
        if kind == "blobs":
            side = min(w, h)
            out[i, :side, :side] = qc.symmetric_blobs(seed + 17 * i, side=side, blobs=max(2, side // 27))
        else:
            out[i] = qc.small_sheet(kind, seed + 17 * i, w, h)
    return out


def draw(rng, c):
    """Case c: its settings (JSON-able), its frames, and why it is left out (or None)."""
    w = int(rng.integers(100, 700)); h = int(rng.integers(90, 500))
    if rng.random() < 0.3: w = (w // 4) * 4
    n = int(rng.integers(1, 5))
    settings = {"quad_decimate": int(rng.choice([1, 1, 2]))}
    if rng.random() < 0.3: settings["refine_edges"] = 0
    if rng.random() < 0.5: settings["max_nmaxima"] = int(rng.integers(4, 13))
    if rng.random() < 0.5: settings["min_component_px"] = int(rng.choice([5, 25, 60, 200]))
    if rng.random() < 0.2: settings["min_cluster_pixels"] = int(rng.choice([5, 24, 50, 120]))
    if rng.random() < 0.3: settings["max_line_fit_mse"] = float(rng.choice([0.3, 1.0, 4.0, 10.0, 30.0]))
    if rng.random() < 0.2: settings["cos_critical_rad"] = float(rng.choice([0.5, 0.8, 0.984807753012208, 0.999]))
    ka, kb = (str(k) for k in rng.choice(KINDS, 2))
    sa, sb = int(rng.integers(1, 1000)), int(rng.integers(1, 1000))
    x0, y0 = int(rng.integers(0, w // 2)), int(rng.integers(0, h // 2))
    frames = cc.side_by_side(content(ka, w, h, n, sa), content(kb, w, h, n, sb), x0, y0)
    info = {"case": c, "w": w, "h": h, "n": n, "settings": settings, "kinds": [ka, kb], "seeds": [sa, sb], "x0": x0, "y0": y0}
    dec = settings["quad_decimate"]
    qw, qh = w // dec, h // dec
    ccap = max(1024, qw * qh // 32)
    table = 1
    while table < 2 * ccap:
        table *= 2
    left = None
    for i in range(n):
        th, lab, sz = cc.oracle_stages(pyoracle, frames[i], dec)
        cl, pts, _ = pyoracle.clusters(th, lab, sz, settings.get("min_component_px", 25))
        lo, hi = cc.gate(qw, qh, settings.get("min_cluster_pixels", 24))
        kept = int(((cl[:, 3] >= lo) & (cl[:, 3] <= hi)).sum()) if len(cl) else 0
        if len(cl) > table: left = left or "pairs %d > table %d" % (len(cl), table)
        if kept > ccap: left = left or "kept %d > cluster list %d" % (kept, ccap)
    return info, frames, left


def run(cases, seed):
    rng = np.random.default_rng(seed)
    bad = left_out = total = 0
    for c in range(cases):
        info, frames, left = draw(rng, c)
        if os.environ.get("STRESS_LOG"):
            with open(os.environ["STRESS_LOG"], "a") as lf:
                lf.write(json.dumps(dict(info, left_out=left)) + "\n")
        if left:
            left_out += 1
            print(json.dumps(dict(info, left_out=left)))
            continue
        n, h, w = frames.shape
        cfg = qc.config(w, h, info["settings"])
        det = qc.detector(w, h, n + c % 3, info["settings"])   # the handle is sized for more frames than the call brings
        got = det.quads(frames)
        det.close()
        for i in range(n):
            want = qc.sort_quads(pyoracle.quads_to_np(pyoracle.quads(frames[i], cfg)))
            have = qc.sort_quads(pyoracle.quads_to_np(got[i]))
            total += len(want)
            if want.shape != have.shape or want.tobytes() != have.tobytes():
                bad += 1
                print(json.dumps(dict(info, frame=i, want=len(want), have=len(have))))
    print(json.dumps({"cases": cases, "left_out": left_out, "oracle_quads": total, "mismatching_frames": bad}))
    if left_out * 10 > cases:
        print(json.dumps({"error": "more than a tenth of the cases left out"}))
        return bad + 1
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 60, int(sys.argv[2]) if len(sys.argv) > 2 else 1) else 0)
