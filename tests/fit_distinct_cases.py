"""Frames and CPU-side bookkeeping of the distinct-points tests of the quad fit (tests/test_fit_distinct_host.py for the premise,
tests/test_gpu_fit_distinct.py on the device).  Nothing here touches the GPU.

The premise: k_emit2 stores the two points a straight edge emits at one half-pixel as one word, and nothing else puts a coordinate
into a cluster twice — so the points that reach the fit are distinct, and its front half (k_quads.hip: FitArgs::distinct) sorts
them without a tie-break and without the search for duplicates behind the sort.  `twin_positions` restates, in numpy and from the
oracle's labels, where the emission rule doubles a coordinate; the host test holds the oracle's clusters against it."""
import json

import numpy as np

import cluster_cases as cc
import emit_row_cases as er
import twin_cases as tc

CLUSTER_ROOM = 8192   # (tests/test_gpu_twin_points.py: the oracle counts every component pair towards max_clusters_per_frame)


def noise_frame(w=192, h=96, seed=12):
    """a ramp of +-24 grey levels across the frame under noise of +-3: every 4 x 4 threshold tile has contrast, nothing is straight"""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(-24, 24, w)[None, :] * np.ones((h, 1))
    return np.clip(np.rint(128 + ramp) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)


def host_frames():
    """(name, frame, min_component_px) of every frame the premise is checked on"""
    out = []
    for mcp in tc.EDGE_MIN_COMPONENT:
        out += [(f"twin {name} mcp {mcp}", f, mcp) for name, f in tc.edge_frames().items()]
    out += [(f"twin gate {g}", tc.gate_frame(g), 1) for g in sorted(tc.GATES)]
    for w, h in er.SIZES:
        for mcp in er.MIN_COMPONENT:
            out += [(f"rows {w}x{h} {name} mcp {mcp}", f, mcp) for name, f in er.frames(w, h).items()]
    w, h, mcp, frames = er.rim_noise()
    out += [(f"rows {w}x{h} {name} mcp {mcp}", f, mcp) for name, f in frames.items()]
    out += [(f"noise 192x96 mcp {mcp}", noise_frame(), mcp) for mcp in (5, 25)]
    return out


def _key(a, b):
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    return (np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b)


def twin_positions(th, lab, sz, min_component_px):
    """(cluster key, x, y) of every half-pixel the emission rule produces twice: (2x+1, 2y+1) comes from direction (1,1) of pixel (x, y)
    and from direction (-1,1) of pixel (x+1, y), both emitting pixels (columns 1..w-2, rows 1..h-2), when both pairs are pairs of
    opposite colours in components of at least min_component_px pixels and join the same two components."""
    h, w = th.shape
    ok = (th != 127) & (sz.astype(np.int64) >= min_component_px)
    t = th.astype(np.int32)
    ys, xs = np.mgrid[1:h - 1, 1:w - 2]          # x + 1 <= w - 2
    a, b = (ys, xs), (ys + 1, xs + 1)            # (1,1) of (x, y)
    c, d = (ys, xs + 1), (ys + 1, xs)            # (-1,1) of (x + 1, y)
    k1, k2 = _key(lab[a], lab[b]), _key(lab[c], lab[d])
    m = ok[a] & ok[b] & (t[a] + t[b] == 255) & ok[c] & ok[d] & (t[c] + t[d] == 255) & (k1 == k2)
    return k1[m], 2 * xs[m] + 1, 2 * ys[m] + 1


def cluster_points(oracle, frame, min_component_px):
    """the oracle's clusters of the frame, ungated: (keys [nc], counts [nc], cluster index / x / y / gx / gy of every point), and the
    stages they came from"""
    th, lab, sz = cc.oracle_stages(oracle, frame)
    cl, pts, ov = oracle.clusters(th, lab, sz, min_component_px)
    assert not ov
    counts = cl[:, 3].astype(np.int64)
    assert np.array_equal(cl[:, 2].astype(np.int64), np.cumsum(counts) - counts) and counts.sum() == len(pts)
    keys = (cl[:, 0].astype(np.uint64) << np.uint64(32)) | cl[:, 1].astype(np.uint64)
    ci = np.repeat(np.arange(len(cl), dtype=np.int64), counts)
    return (th, lab, sz), keys, counts, (ci, pts["x"].astype(np.int64), pts["y"].astype(np.int64), pts["gx"].astype(np.int64),
                                           pts["gy"].astype(np.int64))


# ---- the device cases ------------------------------------------------------------------------------------------------------------------
def _outline(w, h, rects, skew):
    """nested skewed outlines as tests/test_gpu_seq_front.py draws them, of sides (sx, sy) each"""
    im = np.full((h, w), 40, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    cx, cy = w // 2, h // 2
    for k, (sx, sy) in enumerate(rects):
        im[(np.abs((xx - cx) - skew * (yy - cy)) < sx / 2) & (np.abs(yy - cy) < sy / 2)] = 215 if k % 2 == 0 else 40
    return im


def large_class_frames():
    """720 x 656: its perimeter gate, 3 (2 w + 2 h) = 8 256 points, admits the two largest classes that sort in LDS (4 097..8 192 and
    8 193..16 384 points).  One outline of 696 x 652 pixels, whose 8 116 points fourteen notches of two pixels' depth in its top edge
    (eight points each) bring to 8 228, and one of 400 x 400.  The large one is of the 8 193..16 384 class only where every point is
    stored on its own; 1280 x 800 has room for an outline that is of that class in distinct coordinates too (1256 x 792 pixels: 12 308
    points, 8 248 coordinates; the gate there is 12 480)."""
    f = _outline(720, 656, ((696, 652), (400, 400)), 0.03)
    top = int(np.argmax(f[:, 360] == 215))   # first bright row at the centre column
    f[top:top + 2, 60 + 8 * np.arange(14)] = 40
    return {"large720": f[None], "large1280": _outline(1280, 800, ((1256, 792), (500, 500)), 0.02)[None]}


def distinct_edge_frames():
    """The outlines of tests/test_gpu_seq_front.py (their point counts straddle the class edges, which is where the device files them
    when it stores every point on its own) drawn larger: here the counts of DISTINCT coordinates, 8.6 per pixel of side, lie just
    below (first frame) and just above (second frame) 256, 512, 1024, 2048 and 4096 — where the device files them with twins merged."""
    from test_gpu_seq_front import _nested
    return np.stack([_nested(704, 560, (466, 232, 116, 58, 29), 352, 280, 0.15), _nested(704, 560, (484, 243, 122, 61, 31), 352, 280, 0.15)])


def device_cases():
    """name -> (frames [n][h][w], settings of the handle)"""
    from test_gpu_seq_front import _frames as seq_frames   # the generators at the class edges; bars and spokes for the bitonic fallback
    cases = {}
    for mcp in tc.EDGE_MIN_COMPONENT:
        cases[f"twin_mcp{mcp}"] = (np.stack(list(tc.edge_frames().values())), dict(min_component_px=mcp))
    for g in sorted(tc.GATES):   # a cluster of 24 (50) points and fewer words than that
        cases[f"gate{g}"] = (tc.gate_frame(g)[None], dict(min_component_px=1, min_cluster_pixels=g))
    for w, h in er.SIZES:
        for mcp in er.MIN_COMPONENT:
            cases[f"rows{w}x{h}_mcp{mcp}"] = (np.stack(list(er.frames(w, h).values())), dict(min_component_px=mcp))
    w, h, mcp, frames = er.rim_noise()
    cases["rows_rim_noise"] = (np.stack(list(frames.values())), dict(min_component_px=mcp))
    for mcp in (5, 25):
        cases[f"noise_mcp{mcp}"] = (noise_frame()[None], dict(min_component_px=mcp))
    seq = seq_frames()
    for name in ("edges640", "edges272", "shapes640"):
        cases[name] = (seq[name], {})
    cases["dedges704"] = (distinct_edge_frames(), {})
    cases["three640"] = (np.stack([seq["edges640"][0], seq["shapes640"][0], seq["edges640"][1]]), {})   # one handle of three
    for name, f in large_class_frames().items():
        cases[name] = (f, {})
    for name in cases:
        cases[name][1].setdefault("max_clusters_per_frame", CLUSTER_ROOM)
    return cases


DET_COLS = 14   # family, id, hamming, margin (as float32), centre, corners


def dets_np(rows):
    """detections (dicts of the oracle or objects of the library, already reduced to tuples) as one float64 array"""
    return np.asarray(rows, np.float64).reshape(-1, DET_COLS)


def oracle_expectations(oracle, frames, settings):
    """per frame: the oracle's quads as sorted records, its detections, its status word"""
    from chalkydri_amd import default_config
    n, h, w = frames.shape
    cfg = default_config(w, h, **settings)
    quads, dets, status = [], [], []
    for i in range(n):
        q = oracle.quads_to_np(oracle.quads(frames[i], cfg))
        quads.append(q[np.lexsort((q[:, 10], q[:, 9]))] if len(q) else q)
        want, st = oracle.detect(frames[i], cfg)
        dets.append(dets_np([[d["family"], d["id"], d["hamming"], np.float32(d["margin"]), *d["c"], *np.asarray(d["p"]).reshape(-1)] for d in want]))
        status.append(st)
    return quads, dets, np.asarray(status, np.uint32)


def save_cases(path, oracle):
    """everything a run on the device needs, in one .npz: frames, settings, expectations.  Returns what the conditions on the inputs
    are checked on: name -> [(points, distinct coordinates)] of the kept clusters, and name -> number of quads."""
    data, sizes, nquads = {}, {}, {}
    for name, (frames, settings) in device_cases().items():
        quads, dets, status = oracle_expectations(oracle, frames, settings)
        data["f_" + name] = frames
        data["s_" + name] = np.frombuffer(json.dumps(settings).encode(), np.uint8)
        data["st_" + name] = status
        for i in range(len(frames)):
            data[f"q_{name}_{i}"], data[f"d_{name}_{i}"] = quads[i], dets[i]
        nquads[name] = sum(len(q) for q in quads)
        sizes[name] = []
        lo, hi = cc.gate(frames.shape[2], frames.shape[1], settings.get("min_cluster_pixels", 24))
        for f in frames:
            _, _, counts, (ci, x, y, _, _) = cluster_points(oracle, f, settings.get("min_component_px", 25))
            distinct = np.bincount(np.unique(np.stack([ci, x, y], 1), axis=0)[:, 0], minlength=len(counts)) if len(ci) else np.zeros(0, np.int64)
            sizes[name] += [(int(c), int(u)) for c, u in zip(counts, distinct) if lo <= c <= hi]
    np.savez(path, **data)
    return sizes, nquads
