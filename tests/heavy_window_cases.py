"""Inputs of the heavy-window parity test of the split quad fit's middle kernel (tests/test_gpu_heavy_windows.py;
tests/test_heavy_window_cases_host.py proves on the CPU that the cases reach what they name).  Nothing here touches the GPU.

k_chunk (chalkydri_amd/csrc/k_chunk.hip) looks 1 / W of a window up in a table whose size is the largest weight sum a window can
have — 41 points of the weight image's ceiling, 362 — and its running sums are sized by the same ceiling.  The frames of
tests/span_cases.py have gradients of 175 grey levels; these have full-contrast edges (0 against 255) along an axis, at 45 degrees
and at a shallow angle, so their points carry the heaviest weights a frame can give: 256 on an axis-parallel edge (gx = 255, gy = 0),
361 = isqrt(2 * 255^2) + 1 on a diagonal one.  Each frame is one dark square on a white sheet: ONE cluster at the fit, which becomes
the frame's one quad, so CK_EXT_BASE = b puts point i of the sorted, de-duplicated cluster at position b + CK_EXT_PRE + i
(tests/span_cases.py), and the bases below put the cluster's heaviest window across each boundary between two waves of the span
k_chunk loads (positions 256, 512 and 768 of its 1 024) and across a boundary between two spans.

The weights and the window sums are restated here from oracle/detector.c (angle_key, the duplicate removal, the weight formula of
fit_quad) on the points pyoracle.clusters returns, because the oracle's readout holds neither."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import quad_cases as qc
import span_cases as sc
from quad_cases import EXIT, FOUND, KSZ, QUAD, UNIQUE

SHEET = 352
WEIGHT_CEILING = 362             # isqrt(255^2 + 255^2) + 1 = 361 is the most the formula gives; 362 is the bound the kernels are written to
WINDOW = 41                      # 2 * 20 + 1 points
WAVE_EDGES = (256, 512, 768)     # positions of the loaded span at which the next wave's four-point runs begin


def square(side, deg, cx=0.0, cy=0.0, sheet=SHEET):
    """One black (0) square of `side` px, turned by `deg` degrees about the sheet's middle + (cx, cy), on a white (255) sheet: a
    pixel is black when its centre lies inside."""
    y, x = np.mgrid[0:sheet, 0:sheet] + 0.5
    x, y = x - sheet / 2 - cx, y - sheet / 2 - cy
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    m = (np.abs(x * c + y * s) < side / 2) & (np.abs(-x * s + y * c) < side / 2)
    return np.where(m, 0, 255).astype(np.uint8)


# (name, side, degrees, centre offset) and what was measured on the restatement below when the cases were written:
# points after duplicate removal, ksz, maxima, the largest point weight, the largest sum of a window of 41, the index of the
# point in the middle of the first such window
CASES = [
    ("axis", 150.0, 0.0, (0.3, 0.2)),
    ("diagonal", 150.0, 45.0, (0.3, 0.2)),
    ("shallow", 150.0, 7.0, (0.3, 0.2)),
]
PINNED = {
    "axis": (1200, 20, 4, 361, 10811, 130),       # (the corners' pixels see both edges: 361 there, 256 along the edges)
    "diagonal": (1692, 20, 570, 361, 14801, 443),  # 14 801 = 41 * 361: the heaviest window a frame can hold
    "shallow": (1336, 20, 85, 361, 11861, 508),
}


def frames():
    return np.ascontiguousarray(np.stack([square(side, deg, *off) for _, side, deg, off in CASES]), np.uint8)


# ---- the oracle's sort and weights, restated -------------------------------------------------------------------------------------------
def angle_keys(x, y):
    """oracle/detector.c: angle_key of every point (x, y in half pixels) about the bounding box's middle, as Python integers."""
    xmin, xmax, ymin, ymax = int(x.min()), int(x.max()), int(y.min()), int(y.max())
    keys = []
    for px, py in zip(x.tolist(), y.tolist()):
        dx, dy = 4 * px - 2 * (xmin + xmax) - 1, 4 * py - 2 * (ymin + ymax) + 1
        ax, ay = abs(dx), abs(dy)
        if dy < 0:
            if dx < 0:
                oct_, inv, num, den = (0, 0, ay, ax) if ay <= ax else (1, 1, ax, ay)
            else:
                oct_, inv, num, den = (2, 0, ax, ay) if ay > ax else (3, 1, ay, ax)
        else:
            if dx > 0:
                oct_, inv, num, den = (4, 0, ay, ax) if ay <= ax else (5, 1, ax, ay)
            else:
                oct_, inv, num, den = (6, 0, ax, ay) if ay > ax else (7, 1, ay, ax)
        frac = (num << 30) // den
        if inv:
            frac = (1 << 30) - frac
        keys.append((oct_ << 57) | (frac << 26) | (px << 13) | py)
    return keys


def point_weights(frame, x, y):
    """fit_quad's weight of the points (x, y) in half pixels: isqrt(gx^2 + gy^2) + 1 of the pixel ((x + 1) >> 1, (y + 1) >> 1), 1
    on the image's rim."""
    h, w = frame.shape
    im = frame.astype(np.int64)
    ix, iy = (x + 1) >> 1, (y + 1) >> 1
    inside = (ix > 0) & (ix + 1 < w) & (iy > 0) & (iy + 1 < h)
    cx, cy = np.clip(ix, 1, w - 2), np.clip(iy, 1, h - 2)
    gx, gy = im[cy, cx + 1] - im[cy, cx - 1], im[cy + 1, cx] - im[cy - 1, cx]
    return np.where(inside, np.array([math.isqrt(int(v)) for v in gx * gx + gy * gy], np.int64) + 1, 1)


def heaviest_window(oracle, frame):
    """(points after duplicate removal, largest point weight, largest sum of a window of 41 consecutive points of the sorted cluster
    (the cluster is a ring), index of the middle point of the first window that reaches it) of the frame's largest cluster."""
    import cluster_cases as cc
    cfg = qc.config(frame.shape[1], frame.shape[0], {})
    th, lab, sz = cc.oracle_stages(oracle, np.ascontiguousarray(frame), 1, cfg.min_white_black_diff)
    cl, pts, ov = oracle.clusters(th, lab, sz, cfg.min_component_px)
    assert not ov
    k = int(np.argmax(cl[:, 3]))
    p = pts[int(cl[k, 2]):int(cl[k, 2]) + int(cl[k, 3])]
    keys = sorted(set(angle_keys(p["x"].astype(np.int64), p["y"].astype(np.int64))))
    x, y = np.array([(q >> 13) & 0x1FFF for q in keys], np.int64), np.array([q & 0x1FFF for q in keys], np.int64)
    wt = point_weights(frame, x, y)
    n = len(wt)
    ring = np.concatenate([wt[n - WINDOW // 2:], wt, wt[:WINDOW // 2]])
    sums = np.convolve(ring, np.ones(WINDOW, np.int64), "valid")   # sums[i]: the window around point i
    assert len(sums) == n
    return n, int(wt.max()), int(sums.max()), int(np.argmax(sums))


def bases(mid):
    """The four values of CK_EXT_BASE that put point `mid` of a frame's only cluster on position 256, 512 and 768 of the span
    k_chunk loads (it loads from KOFF positions in front of the span it decides) and on the first position of a span."""
    out = []
    for target in [e - sc.KOFF for e in WAVE_EDGES] + [0]:
        b = (target - sc.EXT_PRE - mid) % sc.SPAN
        out.append(b)
        assert 0 <= b <= sc.BASE_MAX and (b + sc.EXT_PRE + mid) % sc.SPAN == target
    return out


def check(oracle):
    """(figures {name: (points, ksz, maxima, largest weight, largest window sum, its middle)}, [sorted quads per frame]): asserted
    against PINNED — a change of the frames that loses a figure fails here."""
    fig, quads = {}, []
    for (name, _, _, _), f in zip(CASES, frames()):
        rd, q = qc.trace(oracle, f, {})
        live = rd[rd[:, EXIT] >= 6]
        assert len(live) == 1 and live[0, EXIT] == QUAD and len(q) == 1, "%s: clusters at the fit %s, quads %d" % (name, live.tolist(), len(q))
        n, wmax, smax, mid = heaviest_window(oracle, f)
        assert n == int(live[0, UNIQUE]), "%s: the restated sort keeps %d points, the oracle %d" % (name, n, int(live[0, UNIQUE]))
        fig[name] = (n, int(live[0, KSZ]), int(live[0, FOUND]), wmax, smax, mid)
        assert fig[name] == PINNED[name], "%s: measured %s, pinned %s" % (name, fig[name], PINNED[name])
        assert n >= 240 and fig[name][1] == 20                        # windows of 41 points
        assert wmax <= WEIGHT_CEILING and smax <= WINDOW * WEIGHT_CEILING
        quads.append(q)
    return fig, quads
