"""Inputs and CPU-side bookkeeping of the gradient-cluster parity tests (tests/test_gpu_clusters.py on the device,
tests/test_cluster_cases_host.py for the proof that the cases reach what they name).  Nothing here touches the GPU.

The kernels under test (chalkydri_amd/csrc/k_clusters.hip) cut a frame into 64 x 16 emit tiles; a (tile, component pair) is one
RUN of the temp array, k_scan keeps the clusters with max(24, min_cluster_pixels) <= points <= 3 * (2 qw + 2 qh), and k_scatter
copies runs of 1..64 points on 16-lane groups and longer ones in rounds of 256.  `emit_stats` restates the emit rule in numpy
so that a case can say how many runs it has and how long they are WITHOUT the device; the expected clusters themselves always
come from the oracle (oracle/pyoracle.py)."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_gpu_segment import _frames as _seg_frames  # noqa: E402  (the content kinds of the segmentation tests)

ETW, ETH = 64, 16            # emit tile of k_emit2
CCL_TW, CCL_TH = 128, 32     # tile of the segmentation stage: a component that touches no tile ring is "interior"
RUN_EDGES = (16, 17, 64, 65, 256, 257)   # run lengths either side of k_scatter's thresholds
RUN_BINS = ((1, 16), (17, 64), (65, 256), (257, 1 << 30))


# ---- frame builders ------------------------------------------------------------------------------------------------------------
def tags_fit(w, h):
    """The renderer places three tags of side >= 24: it needs some room."""
    return w >= 120 and h >= 90


def frame(kind, w, h, seed):
    """One [h][w] uint8 frame of a content kind of tests/test_gpu_segment.py ('tags' = its rendered scenes)."""
    return _seg_frames("synth" if kind == "tags" else kind, w, h, 1, seed)[0]


def frames(kind, w, h, n, seed):
    """n frames of one kind, every frame from its own seed."""
    return np.stack([frame(kind, w, h, seed + 17 * i) for i in range(n)])


def comb(w, h, x0, y0, tooth_rows, bar_rows=3, tooth_w=2, gap=3, bumps=0, fg=220, bg=40, into=None):
    """A bar of `bar_rows` rows with one tooth per entry of `tooth_rows` hanging from it (that many rows long, tooth_w wide, `gap`
    apart), top-left corner at (x0, y0); `bumps` one-pixel bumps sit on top of the bar.  The comb is one white component, what
    surrounds it one black one, so the frame's large cluster is theirs and its size follows the outline: six points per tooth row,
    two per bump."""
    im = np.full((h, w), bg, np.uint8) if into is None else into
    teeth = len(tooth_rows)
    bar_len = teeth * tooth_w + (teeth - 1) * gap
    im[y0:y0 + bar_rows, x0:x0 + bar_len] = fg
    for t, rows in enumerate(tooth_rows):
        xs = x0 + t * (tooth_w + gap)
        im[y0 + bar_rows:y0 + bar_rows + rows, xs:xs + tooth_w] = fg
    for k in range(bumps):
        im[y0 - 1, x0 + 2 + 6 * k] = fg
    return im


def _dot_lattices(mask):
    """White dots inside `mask` and dark dots outside it, on two interleaved 4-pixel lattices, each only where its whole 3 x 3
    neighbourhood lies on its own side (so a dot is an isolated one-pixel component and never touches the region's edge)."""
    h, w = mask.shape
    yy, xx = np.mgrid[0:h, 0:w]
    pad = np.pad(mask, 1, mode="edge")
    inside = np.ones_like(mask)
    outside = np.ones_like(mask)
    for dy in range(3):
        for dx in range(3):
            nb = pad[dy:dy + h, dx:dx + w]
            inside &= nb
            outside &= ~nb
    white = inside & (xx % 4 == 2) & (yy % 4 == 2)
    dark = outside & (xx % 4 == 0) & (yy % 4 == 0)
    return white, dark


def region_mask(w, h, x0, y0, rw, rows, rem=0):
    """`rows` full rows of rw pixels from (x0, y0), then `rem` more pixels on the next row."""
    m = np.zeros((h, w), bool)
    m[y0:y0 + rows, x0:x0 + rw] = True
    m[y0 + rows, x0:x0 + rem] = True
    return m


def _region_dark(x0, y0, rw, t):
    rows, rem = divmod(t, rw)
    m = region_mask(x0 + rw + 6, y0 + rows + 6, x0, y0, rw, rows, rem)
    return int(m.sum()) - int(_dot_lattices(m)[0].sum())


def region_shape_for(target, x0, y0, rw):
    """(rows, rem) of a region_mask at (x0, y0), rw wide, whose dark pixels (mask minus its white dots) number exactly `target`.
    One more pixel is one more dark pixel, less the at most one dot whose 3 x 3 neighbourhood it completes: the count never falls
    and never skips a value, so a bisection over the pixel count finds it."""
    lo, hi = target, 2 * target + 16 * rw
    while lo < hi:
        mid = (lo + hi) // 2
        if _region_dark(x0, y0, rw, mid) < target:
            lo = mid + 1
        else:
            hi = mid
    assert _region_dark(x0, y0, rw, lo) == target
    return divmod(lo, rw)


def dotted_region(w, h, regions, dark=40, light=215, dark_dot=60, light_dot=190):
    """A light field with dark regions (`regions`: (x0, y0, rw, target) each, the region's black component gets exactly `target`
    pixels).  The regions carry isolated brighter pixels and the field isolated darker ones every 4 px: every 4 x 4 threshold tile
    then has contrast, so a region is ONE black component (without the dots its flat interior would threshold to 127 and only a rim
    would remain).  The regions must keep 3 px from each other and 2 px from the frame."""
    mask = np.zeros((h, w), bool)
    for x0, y0, rw, target in regions:
        rows, rem = region_shape_for(target, x0, y0, rw)
        assert x0 >= 2 and y0 >= 2 and x0 + rw <= w - 2 and y0 + rows + 1 <= h - 2, "region leaves the frame"
        m = region_mask(w, h, x0, y0, rw, rows, rem)
        grown = np.pad(mask, 3)[0:h + 6, 0:w + 6]
        near = np.zeros_like(mask)
        for dy in range(7):
            for dx in range(7):
                near |= grown[dy:dy + h, dx:dx + w]
        assert not (near & m).any(), "regions too close"
        mask |= m
    white, dk = _dot_lattices(mask)
    im = np.where(mask, dark, light).astype(np.uint8)
    im[white] = light_dot
    im[dk] = dark_dot
    return im


def checker_patch(w, h, x0, y0, pw, ph):
    """A one-pixel checkerboard rectangle in a flat frame of value 128."""
    im = np.full((h, w), 128, np.uint8)
    yy, xx = np.mgrid[y0:y0 + ph, x0:x0 + pw]
    im[y0:y0 + ph, x0:x0 + pw] = (((yy + xx) & 1) * 255).astype(np.uint8)
    return im


def side_by_side(a, b, x0, y0):
    """`a` with the (w / 2) x (h / 2) window of `b` at (x0, y0) pasted over it: two kinds of content in one frame."""
    out = a.copy()
    h, w = a.shape[-2:]
    out[..., y0:y0 + h // 2, x0:x0 + w // 2] = b[..., y0:y0 + h // 2, x0:x0 + w // 2]
    return out


# ---- the oracle's view of a frame ----------------------------------------------------------------------------------------------------
def oracle_stages(oracle, img, dec=1, min_white_black_diff=5):
    """(threshold, labels, sizes) of the image the quad stages run on."""
    img = np.ascontiguousarray(img, np.uint8)
    if dec > 1:
        h, w = img.shape
        q = np.empty((h // dec, w // dec), np.uint8)
        oracle.lib().ora_decimate(C.c_void_p(img.ctypes.data), w, h, w, dec, C.c_void_p(q.ctypes.data))
        img = q
    th = oracle.threshold(img, min_white_black_diff)
    lab, sz = oracle.segment(th)
    return th, lab, sz


def gate(qw, qh, min_cluster_pixels=24):
    """k_scan's gates: the point counts a kept cluster may have."""
    return max(24, min_cluster_pixels), 3 * (2 * qw + 2 * qh)


def cluster_dict(cl, pts, lo=24, hi=1 << 30):
    """{(rep0, rep1): sorted [x, y, gx, gy] rows} of the clusters with lo <= count <= hi (the order of a cluster's points is not
    defined on the device)."""
    out = {}
    for rep0, rep1, start, count in cl:
        if count < lo or count > hi:
            continue
        p = pts[start:start + count]
        arr = np.stack([p["x"].astype(np.int64), p["y"].astype(np.int64), p["gx"].astype(np.int64), p["gy"].astype(np.int64)], 1)
        out[(int(rep0), int(rep1))] = arr[np.lexsort((arr[:, 3], arr[:, 2], arr[:, 1], arr[:, 0]))]
    return out


def oracle_clusters(oracle, img, min_component_px=25, min_cluster_pixels=24, dec=1):
    """The clusters the device must return for `img`: the oracle's, filtered by k_scan's gates."""
    th, lab, sz = oracle_stages(oracle, img, dec)
    cl, pts, ov = oracle.clusters(th, lab, sz, min_component_px)
    assert not ov
    lo, hi = gate(th.shape[1], th.shape[0], min_cluster_pixels)
    return cluster_dict(cl, pts, lo, hi)


def caps_for(wants):
    """cluster_cap / point_cap for det.clusters(): room for the largest of the expected results, and to spare."""
    ncl = max([len(w) for w in wants] + [0])
    npt = max([sum(len(v) for v in w.values()) for w in wants] + [0])
    return ncl + 64, npt + 1024


def check_frame(got, want, tag=""):
    """One frame's device result (cluster records, points) against the expected dict: the same keys, the same sorted points, and
    records whose start / count tile the returned point array without gap or overlap."""
    cl, pts = got
    have = cluster_dict(cl, pts)
    assert len(have) == len(cl), f"{tag}: a cluster key occurs twice"
    assert set(have) == set(want), f"{tag}: cluster keys differ: {len(want)} expected, {len(have)} returned, " \
        f"{len(set(want) - set(have))} missing, {len(set(have) - set(want))} extra"
    for k in want:
        assert np.array_equal(want[k], have[k]), f"{tag}: points of cluster {k} differ ({len(want[k])} vs {len(have[k])})"
    if len(cl):
        order = np.argsort(cl[:, 2], kind="stable")
        starts, counts = cl[order, 2].astype(np.int64), cl[order, 3].astype(np.int64)
        assert starts[0] == 0 and np.array_equal(starts[1:], (starts + counts)[:-1]), f"{tag}: cluster records leave a gap or overlap"
        assert starts[-1] + counts[-1] == len(pts), f"{tag}: the point array is longer than its clusters"
    else:
        assert len(pts) == 0, f"{tag}: points without clusters"


# ---- the emit rule, restated ---------------------------------------------------------------------------------------------------------
class EmitStats:
    """What `emit_stats` returns: kept (clusters inside the gates), pairs (distinct component pairs of the frame), pairs_per_tile
    (array over the 64 x 16 emit tiles, row-major), runs ((tile, pair) runs), run_lengths (of kept clusters' runs), cluster_sizes
    (point counts of ALL clusters)."""

    def __init__(self, kept, pairs, pairs_per_tile, runs, run_lengths, cluster_sizes):
        self.kept, self.pairs, self.pairs_per_tile, self.runs = kept, pairs, pairs_per_tile, runs
        self.run_lengths, self.cluster_sizes = run_lengths, cluster_sizes

    def bins(self):
        return [int(np.count_nonzero((self.run_lengths >= a) & (self.run_lengths <= b))) for a, b in RUN_BINS]

    def edges(self):
        return sorted(int(e) for e in RUN_EDGES if np.any(self.run_lengths == e))

    def line(self):
        ppt = self.pairs_per_tile
        return "kept %d  pairs %d  pairs/tile max %d  runs %d  run bins %s  edges %s" % (
            self.kept, self.pairs, int(ppt.max()) if ppt.size else 0, self.runs, self.bins(), self.edges())


def emit_stats(th, lab, sz, min_component_px=25, min_cluster_pixels=24):
    """Vectorised restatement of the emit rule (for the cases' preconditions only): a point for each of the pairs (1,0), (0,1),
    (-1,1), (1,1) from the pixels 1 <= x <= w-2, 1 <= y <= h-2 whose two members are both != 127, of opposite colour and in
    components of >= min_component_px pixels; key (min label, max label); a point belongs to the emit tile of its first pixel."""
    h, w = th.shape
    lo, hi = gate(w, h, min_cluster_pixels)
    tiles_x, tiles_y = (w + ETW - 1) // ETW, (h + ETH - 1) // ETH
    t = th.astype(np.int32)
    ok_px = (th != 127) & (sz.astype(np.int64) >= min_component_px)
    keys, tiles = [], []
    if w >= 3 and h >= 3:
        ys, xs = np.mgrid[1:h - 1, 1:w - 1]
        tile0 = (ys // ETH) * tiles_x + xs // ETW
        for dx, dy in ((1, 0), (0, 1), (-1, 1), (1, 1)):
            a_ok, b_ok = ok_px[1:h - 1, 1:w - 1], ok_px[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
            m = a_ok & b_ok & (t[1:h - 1, 1:w - 1] + t[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx] == 255)
            la = lab[1:h - 1, 1:w - 1][m].astype(np.uint64)
            lb = lab[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx][m].astype(np.uint64)
            keys.append((np.minimum(la, lb) << np.uint64(32)) | np.maximum(la, lb))
            tiles.append(tile0[m].astype(np.int64))
    keys = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
    tiles = np.concatenate(tiles) if tiles else np.zeros(0, np.int64)
    ukeys, kinv, ksize = np.unique(keys, return_inverse=True, return_counts=True)
    kept_key = (ksize >= lo) & (ksize <= hi)
    # runs: distinct (tile, key)
    run_id = tiles * max(len(ukeys), 1) + kinv
    uruns, rlen = np.unique(run_id, return_counts=True)
    run_tile, run_key = uruns // max(len(ukeys), 1), uruns % max(len(ukeys), 1)
    ppt = np.bincount(run_tile, minlength=tiles_x * tiles_y)
    return EmitStats(int(kept_key.sum()), len(ukeys), ppt, len(uruns), rlen[kept_key[run_key]] if len(uruns) else np.zeros(0, np.int64), ksize)


# ---- the cases (shared by the host and the GPU tests) --------------------------------------------------------------------------------
# a. geometry x content x gate: (w, h, quad_decimate); the emit tile is 64 x 16, so these have a single tile, last column tiles of
# 1, 2 and 3 pixels, a last row tile of one row, and decimated images of 321 x 241 and 130 x 68
GEOMETRY = [(61, 47, 1), (64, 16, 1), (65, 17, 1), (66, 33, 1), (127, 31, 1), (129, 33, 1), (130, 49, 1), (131, 35, 1), (191, 63, 1), (258, 98, 1),
            (640, 480, 1), (642, 482, 2), (260, 136, 2)]
KINDS = ("noise", "blobs", "stripes", "spiral", "tags")
GEOMETRY_MIN_COMPONENT = (25, 5)
GEOMETRY_N, GEOMETRY_SEED = 3, 3


def geometry_kinds(w, h, dec):
    return [k for k in KINDS if k != "tags" or tags_fit(w // dec, h // dec)]


def geometry_frames(w, h, kind):
    return frames(kind, w, h, GEOMETRY_N, GEOMETRY_SEED)


# b. many runs
MANY_RUNS = dict(w=640, h=480, seed=3, min_component_px=1)

# c. batch dealing
DEAL_W, DEAL_H, DEAL_MIN_COMPONENT = 130, 49, 5
DEAL_N = (1, 4, 5, 8, 15, 16, 17, 23, 24)


def deal_frame(j):
    """Frame j of the dealing cases: the kinds take turns, and a window of seeded noise or blobs at a place of its own makes every
    frame different from every other (stripes and spiral are drawn, not seeded)."""
    kind = ("noise", "blobs", "stripes", "spiral")[j % 4]
    other = frame("blobs" if kind == "noise" else "noise", DEAL_W, DEAL_H, 200 + j)
    return side_by_side(frame(kind, DEAL_W, DEAL_H, 100 + j), other, (7 * j) % (DEAL_W // 2), (5 * j) % (DEAL_H // 2))


# d. cluster-size gates.  Upper: 64 x 48, bound 3 * (2 * 64 + 2 * 48) = 672; a comb of three 2-pixel teeth of 33 rows on a 3-row bar is
# a cluster of exactly 672 points, a bump on the bar adds 2, a tooth row less takes 6
UPPER_W, UPPER_H = 64, 48
UPPER_COMBS = {670: dict(tooth_rows=(33, 33, 32), bumps=2), 672: dict(tooth_rows=(33, 33, 33)), 674: dict(tooth_rows=(33, 33, 33), bumps=1)}


def upper_gate_frame(points):
    return comb(UPPER_W, UPPER_H, 8, 6, **UPPER_COMBS[points])


# Lower: bright shapes of a few pixels on a dark frame, at min_component_px = 1.  A 2 x 2 square has 20 neighbour pairs of opposite
# colour, a 2 x 2 square with a fifth pixel beside it 24, a 2 x 3 rectangle 26.
LOWER_W, LOWER_H = 192, 64
LOWER_SHAPES = {20: ((0, 0), (1, 0), (0, 1), (1, 1)), 24: ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0)), 26: ((0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2))}
# where the copies sit: the first of each shape straddles an emit-tile corner (x = 64 or 128, y = 16 or 32 or 48)
LOWER_AT = {20: ((63, 15), (20, 6), (150, 40), (100, 56)), 24: ((127, 31), (40, 24), (170, 8)), 26: ((63, 47), (90, 8), (20, 40), (150, 22), (110, 36))}


def lower_gate_frame():
    im = np.full((LOWER_H, LOWER_W), 40, np.uint8)
    for pts, shape in LOWER_SHAPES.items():
        for x, y in LOWER_AT[pts]:
            for dx, dy in shape:
                im[y + dy, x + dx] = 220
    return im


# e. component-size gate: (min_component_px, w, h); every frame holds regions of m - 1, m and m + 1 dark pixels
COMPONENT_GATE = [(25, 512, 192), (1000, 512, 192), (0x7FFF, 640, 480), (0x8000, 640, 480), (40000, 640, 480), (70000, 800, 600)]


def component_gate_regions(m, w, h):
    """(x0, y0, width, dark pixels) per region.  The small ones come in three placements: inside one 128 x 32 segmentation tile (off
    its ring), across a tile corner, and down a column of tiles (m = 1000: 76 rows, three tile rows; a component of 24..26 pixels cannot
    reach a third tile row, its column crosses one tile edge).  The large ones span dozens of tiles anyway."""
    if m == 25:
        return [(6 + 128 * i, 131, 5, m - 1 + i) for i in range(3)] + [(125 + 128 * i, 30, 6, m - 1 + i) for i in range(3)] + \
               [(440 + 20 * i, 20, 1, m - 1 + i) for i in range(3)]
    if m == 1000:
        return [(6 + 128 * i, 131, 44, m - 1 + i) for i in range(3)] + [(110 + 128 * i, 18, 36, m - 1 + i) for i in range(3)] + \
               [(440 + 20 * i, 50, 14, m - 1 + i) for i in range(3)]
    rw = 200 if w == 640 else 250
    return [(8 + (rw + 12) * i, 8, rw, m - 1 + i) for i in range(3)]


def component_gate_frame(m, w, h):
    return dotted_region(w, h, component_gate_regions(m, w, h))


# f. the 512 entries of k_emit2's LDS table: one-pixel checkerboards at min_component_px = 1 (every dark pixel its own component)
TABLE_W, TABLE_H = 272, 200
TABLE_PATCH = {512: (64, 16, 64, 16), 552: (60, 12, 74, 24)}   # pairs in the fullest emit tile: (x0, y0, width, height) of the patch


def table_frame(pairs):
    return checker_patch(TABLE_W, TABLE_H, *TABLE_PATCH[pairs])


def table_tag_frames():
    """The rendered-tag frames that go before and after a checkerboard frame in its batch (without sensor noise: at
    min_component_px = 1 every noise speck would be a cluster, and 3000 of them are more than the handle's 1700)."""
    from chalkydri_amd import synth
    return synth.render_batch(11, 2, TABLE_W, TABLE_H, 2, min_side=24, max_side=60, noise_amp=0)[0]
