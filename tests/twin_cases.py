"""Hand-drawn frames for the twin-point tests (tests/test_gpu_twin_points.py on the device, tests/test_twin_points_host.py for the
proof that each frame reaches what it is named for).  Nothing here touches the GPU.

A boundary point at half-pixel (2x+1, 2y+1) is emitted twice into one cluster when both diagonals of the 2 x 2 block at (x, y) join
the same two components: by direction (1,1) from pixel (x, y) and by direction (-1,1) from pixel (x+1, y).  k_emit2 stores such a
twin as one word; what the library returns must not show it."""
import numpy as np

import cluster_cases as cc

W, H = 160, 96               # 3 x 6 emit tiles of 64 x 16 (the last column tile 32 wide)
DARK, LIGHT = 40, 220


def _grid(w=W, h=H):
    return np.mgrid[0:h, 0:w]


def vedge(x, w=W, h=H):
    """dark columns [0, x), light columns [x, w): a vertical edge between columns x - 1 and x"""
    im = np.full((h, w), LIGHT, np.uint8)
    im[:, :x] = DARK
    return im


def hedge(y, w=W, h=H):
    im = np.full((h, w), LIGHT, np.uint8)
    im[:y, :] = DARK
    return im


def cross(x, y, w=W, h=H):
    yy, xx = _grid(w, h)
    return np.where((xx < x) ^ (yy < y), DARK, LIGHT).astype(np.uint8)


def checker(cell, w=W, h=H):
    yy, xx = _grid(w, h)
    return np.where(((xx // cell + yy // cell) & 1) == 1, LIGHT, DARK).astype(np.uint8)


def staircase(w=W, h=H):
    """a 45 degree boundary, one pixel per step: no 2 x 2 block on it has uniform rows or columns"""
    yy, xx = _grid(w, h)
    return np.where(yy > xx - 30, DARK, LIGHT).astype(np.uint8)


# name -> frame.  "tile": straight edges across the emit-tile boundaries x = 63|64 and y = 15|16; "rim": edges through the first and
# last emitting columns and rows (1, w - 2, 1, h - 2) and one further out, where one copy of a twin pair has no emitting owner;
# "mixed": twins of different clusters (checkerboards) or no twins at all (the staircase)
def edge_frames():
    f = {"tile v63|64": vedge(64), "tile h15|16": hedge(16), "tile cross": cross(64, 16)}
    for x in (1, 2, W - 2, W - 1):
        f[f"rim v{x - 1}|{x}"] = vedge(x)
    for y in (1, 2, H - 2, H - 1):
        f[f"rim h{y - 1}|{y}"] = hedge(y)
    f["mixed checker2"] = checker(2)
    f["mixed checker3"] = checker(3)
    f["mixed staircase"] = staircase()
    return f


EDGE_MIN_COMPONENT = (25, 1)


def duplicates(want):
    """{key: set of (x, y) that occur twice} of an expected-cluster dict"""
    out = {}
    for k, arr in want.items():
        xy, n = np.unique(arr[:, :2], axis=0, return_counts=True)
        assert n.max() <= 2
        out[k] = {tuple(int(v) for v in p) for p in xy[n == 2]}
    return out


def totals(oracle, img, min_component_px):
    """(logical, physical) point totals of ALL clusters of the frame, whatever their size: what the point capacity is filled by"""
    th, lab, sz = cc.oracle_stages(oracle, img)
    cl, pts, ov = oracle.clusters(th, lab, sz, min_component_px)
    assert not ov
    phys = 0
    for _, _, start, count in cl:
        p = pts[start:start + count]
        phys += len(set(zip(p["x"].tolist(), p["y"].tolist())))
    return len(pts), phys


# Shapes of light pixels on a dark frame whose one cluster (at min_component_px = 1) has exactly `points` points, twins counted
# twice: (points, top row, pixels).  A closed outline away from the frame's edge always has an even count; a shape in rows 0 / 1
# loses the points row 0 would emit, which is where the odd ones come from.
def _rect(a, b, *extra):
    return tuple((x, y) for y in range(b) for x in range(a)) + tuple(extra)


GATE_SHAPES = {23: (0, _rect(1, 5)), 24: (0, _rect(1, 5, (1, 1))), 49: (1, _rect(1, 8, (1, 1))), 50: (0, _rect(4, 8))}
GATE_W, GATE_H = 128, 32
# where the shapes sit: the kept one of each pair straddles the emit-tile boundary x = 63|64
GATE_AT = {23: 20, 24: 63, 49: 100, 50: 62}
GATES = {24: (23, 24), 50: (49, 50)}     # min_cluster_pixels -> (dropped, kept)


def gate_frame(min_cluster_pixels):
    im = np.full((GATE_H, GATE_W), DARK, np.uint8)
    for pts in GATES[min_cluster_pixels]:
        top, shape = GATE_SHAPES[pts]
        for dx, dy in shape:
            im[top + dy, GATE_AT[pts] + dx] = LIGHT
    return im


def cluster_sizes(oracle, img, min_component_px=1):
    """[(logical, distinct coordinates)] of every cluster of the frame, ungated"""
    th, lab, sz = cc.oracle_stages(oracle, img)
    cl, pts, _ = oracle.clusters(th, lab, sz, min_component_px)
    out = []
    for _, _, start, count in cl:
        p = pts[start:start + count]
        out.append((int(count), len(set(zip(p["x"].tolist(), p["y"].tolist())))))
    return sorted(out)
