"""Maxima per cluster on frames of the bench batch, from the oracle's per-cluster readout (CPU only): what the selection of the quad
fit's tail (k_quads.hip, k_tail_body 5a) meets.  usage: python tools/maxima_histogram.py [frames=3] [w=1280] [h=800]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import pyoracle
import quad_cases as qc
from chalkydri_amd import scenes

n = int(sys.argv[1]) if len(sys.argv) > 1 else 3
w = int(sys.argv[2]) if len(sys.argv) > 2 else 1280
h = int(sys.argv[3]) if len(sys.argv) > 3 else 800
frames = scenes.bench_stream(2, n, w, h, 6, noise_amp=3)[0]
rd = np.concatenate([qc.trace(pyoracle, f, {})[0] for f in frames])
found, pts = rd[:, qc.FOUND], rd[:, qc.UNIQUE]
reach = found >= 0
f, p = found[reach], pts[reach]
print("frames", n, "clusters per frame", len(rd) / n, "that reach the maxima", reach.sum() / n)
print("maxima per cluster: median", int(np.median(f)), "mean", round(float(f.mean()), 1), "points per maximum", round(float(p.sum()) / max(1, int(f.sum())), 1))
for t in (10, 32, 64, 128, 256, 512):
    over = f > t
    print("nmax > %3d: %5.2f %% of the clusters (%.1f per frame), mean nmax %.0f, %4.1f %% of the points" %
          (t, 100.0 * over.mean(), over.sum() / n, f[over].mean() if over.any() else 0, 100.0 * p[over].sum() / p.sum()))
print("largest nmax", int(f.max()))
