"""Inputs and CPU-side bookkeeping of the parity tests of the quad fit's back half (tests/test_gpu_quad_back.py on the device,
tests/test_quad_cases_host.py for the proof that the cases reach what they name).  Nothing here touches the GPU.

The back half (chalkydri_amd/csrc/k_quads.hip: k_fit after its sort, k_tail) smooths the line-fit error over a window of ksz =
min(points / 12, 20), takes its local maxima, cuts them to max_nmaxima, searches the 4-subsets of what is left, and puts the winner
through the mean-error, corner, area, angle and winding checks and through edge refinement.  A case is (name, frames [n][h][w],
settings); CONDITIONS[name] checks on the oracle's per-cluster readout (pyoracle.fit_trace) that the frames reach the edge the case
is named for, and returns the figures it measured.  The expected quads always come from the oracle."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

EXIT, POINTS, UNIQUE, KSZ, FOUND, KEPT, TIES, REVERSED = range(8)   # pyoracle.FIT_TRACE_FIELDS
QUAD = 14                                                           # the exit number of a cluster that became a quad
BRIGHT, DARK = 215, 40


# ---- settings ------------------------------------------------------------------------------------------------------------------------
# A case's settings are a JSON-able dict: "families" (names: built-in ones or tests/family_gen.py's), "quad_decimate", and fields of
# ck_config_t.
def _families(settings):
    from chalkydri_amd import family
    import family_gen as fg
    return tuple(family(n) if n.startswith("tag") else fg.make(n) for n in settings.get("families", ("tag36h11",)))


def config(w, h, settings):
    from chalkydri_amd import default_config
    kw = {k: v for k, v in settings.items() if k != "families"}
    return default_config(w, h, families=_families(settings), **kw)


def detector(w, h, n, settings):
    from chalkydri_amd.detector import AprilTagDetector
    kw = {k: v for k, v in settings.items() if k != "families"}
    return AprilTagDetector(w, h, max_batch=n, families=_families(settings), **kw)


# ---- the oracle's view ---------------------------------------------------------------------------------------------------------------
def trace(oracle, frame, settings):
    """(readouts [clusters][8], quads [k][11] sorted by (rep0, rep1)) of one frame under the settings."""
    import cluster_cases as cc
    h, w = frame.shape
    cfg = config(w, h, settings)
    dec = max(1, int(cfg.quad_decimate))
    q = np.ascontiguousarray(frame)
    if dec > 1:
        import ctypes as C
        q = np.empty((h // dec, w // dec), np.uint8)
        oracle.lib().ora_decimate(C.c_void_p(np.ascontiguousarray(frame).ctypes.data), w, h, w, dec, C.c_void_p(q.ctypes.data))
    th, lab, sz = cc.oracle_stages(oracle, q, 1, cfg.min_white_black_diff)
    cl, pts, ov = oracle.clusters(th, lab, sz, cfg.min_component_px)
    assert not ov
    tr = oracle.fit_trace(frame, cfg, cl, pts, quad_img=q)
    rd = np.array([t for t, _ in tr], np.int64).reshape(-1, 8)
    quads = sort_quads(oracle.quads_to_np([qd for _, qd in tr if qd is not None]))
    return rd, quads


def sort_quads(a):
    return a[np.lexsort((a[:, 10], a[:, 9]))] if len(a) else a


def frame_index(frames):
    """index[i] = the first frame of the call equal to frame i (a repeated frame shares its oracle result)"""
    first, index = {}, []
    for i, f in enumerate(frames):
        index.append(first.setdefault(f.tobytes(), i))
    return index


def case_trace(oracle, frames, settings):
    """(readouts of all distinct frames stacked, {frame index: sorted quads} of the distinct frames, index)"""
    index = frame_index(frames)
    rds, quads = [], {}
    for i in sorted(set(index)):
        rd, q = trace(oracle, frames[i], settings)
        rds.append(rd)
        quads[i] = q
    return np.concatenate(rds), quads, index


# ---- drawing -------------------------------------------------------------------------------------------------------------------------
SMALL_W, SMALL_H, SMALL_GRID = 320, 240, 20
SMALL_HALF = [round(1.0 + 0.2 * k, 1) for k in range(24)]   # half-sizes 1.0 .. 5.6 px
SMALL_SETTINGS = {"min_component_px": 5}


def small_sheet(kind, seed, w=SMALL_W, h=SMALL_H):
    """Dark squares ('squares') or discs ('discs') of every half-size of SMALL_HALF on a bright sheet, one per cell of a 20 px grid,
    each at a random sub-pixel offset and (squares) rotation.  A pixel is dark when its centre lies inside the shape: hard edges,
    which is what leaves clusters with as few as two maxima.  (Bright shapes on a dark sheet would all leave at the border-direction
    test under tag36h11.)"""
    rng = np.random.default_rng(seed)
    im = np.full((h, w), BRIGHT, np.uint8)
    g = SMALL_GRID
    y, x = np.mgrid[0:g, 0:g] + 0.5
    k = 0
    for cy in range(h // g):
        for cx in range(w // g):
            r = SMALL_HALF[k % len(SMALL_HALF)]
            k += 1
            ox, oy = g / 2 + rng.uniform(-1, 1), g / 2 + rng.uniform(-1, 1)
            a = rng.uniform(0, np.pi / 2)
            if kind == "discs":
                m = (x - ox) ** 2 + (y - oy) ** 2 < r * r
            else:
                ca, sa = np.cos(a), np.sin(a)
                m = (np.abs((x - ox) * ca + (y - oy) * sa) < r) & (np.abs(-(x - ox) * sa + (y - oy) * ca) < r)
            im[cy * g:(cy + 1) * g, cx * g:(cx + 1) * g][m] = DARK
    return im


def small_frames():
    return np.stack([small_sheet("squares", 3), small_sheet("discs", 2)])


# ---- mse_window: the small sheets under a max_line_fit_mse at which some cluster's four lines each pass and their mean does not ----------
# (found by search_mse_window over both sheets; a cluster of sz points leaves at exit 8 for max_mse * sz / (sz + 4) < its error <= max_mse)
MSE_WINDOW = [(0.09173630764819175, (0,)), (0.17131893829232733, (0, 1)), (0.2459535083043446, (1,))]   # (max_line_fit_mse, frames of small_frames())


def search_mse_window(oracle, lo=0.03, hi=1.5, steps=120):
    """The sweep that found MSE_WINDOW: (value, frame, clusters at exit 8) wherever there is one."""
    out = []
    for v in np.geomspace(lo, hi, steps):
        for i, f in enumerate(small_frames()):
            rd, _ = trace(oracle, f, dict(SMALL_SETTINGS, max_line_fit_mse=float(v)))
            if (rd[:, EXIT] == 8).any():
                out.append((float(v), i, int((rd[:, EXIT] == 8).sum())))
    return out


# ---- noise: rendered tag scenes with sensor noise ------------------------------------------------------------------------------------------
NOISE_W, NOISE_H, NOISE_CONFIG, NOISE_FRAMES = 320, 240, 15, (6, 8, 14)   # no single frame of the first 16 meets every condition under every setting
NOISE_SETTINGS = [{"max_nmaxima": m, "quad_decimate": d, "refine_edges": r} for m in (4, 10, 12) for d in (1, 2) for r in (0, 1)] + \
                 [{"max_nmaxima": 10, "quad_decimate": 1, "refine_edges": 1, "cos_critical_rad": 0.5}]


def noise_frames(w=NOISE_W, h=NOISE_H, which=NOISE_FRAMES):
    from chalkydri_amd import synth
    kw = dict(noise_amp=3)
    if min(w, h) < 300:
        kw.update(min_side=24, max_side=max(24, min(w, h) // 3))
    return np.stack([synth.render_batch(NOISE_CONFIG, 1, w, h, 4, first=i, **kw)[0][0] for i in which])


# ---- ties: frames equal to their own transpose -----------------------------------------------------------------------------------------------
TIES_SIDE = 160
TIES_SETTINGS = {"min_component_px": 5}


def symmetric_blobs(seed, side=TIES_SIDE, blobs=6):
    """Dark lobed blobs (radius r (1 + 0.35 cos(k angle + phase))) on a bright sheet, each drawn with its mirror image in the main
    diagonal, under noise of +-3 that is mirrored too: the frame equals its transpose, so a cluster that straddles the diagonal has
    its maxima in mirrored pairs whose smoothed errors differ by summation order alone, and are sometimes equal to the bit."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    im = np.full((side, side), BRIGHT, np.int64)
    for _ in range(blobs):
        r, k, ph = rng.uniform(8, 22), int(rng.integers(3, 9)), rng.uniform(0, 2 * np.pi)
        cx, cy = rng.uniform(r, side - r), rng.uniform(r, side - r)
        m = np.hypot(xx - cx, yy - cy) < r * (1 + 0.35 * np.cos(k * np.arctan2(yy - cy, xx - cx) + ph))
        im[m | m.T] = DARK
    im = np.minimum(im, im.T)
    nz = np.triu(rng.integers(-3, 4, (side, side)))
    nz = nz + np.triu(nz, 1).T
    out = np.clip(im + nz, 0, 255).astype(np.uint8)
    assert np.array_equal(out, out.T)
    return out


# ---- border: quads whose refinement samples leave the image ----------------------------------------------------------------------------------
BORDER_W, BORDER_H = 200, 160


def border_frame(off):
    """Four dark 44 x 50 rectangles on a bright sheet, one `off` px from each side of the frame."""
    w, h = BORDER_W, BORDER_H
    im = np.full((h, w), BRIGHT, np.uint8)
    im[off:off + 44, 30:80] = DARK                      # top (50 wide, 44 high)
    im[h - off - 44:h - off, 120:170] = DARK            # bottom
    im[90:140, off:off + 44] = DARK                     # left (44 wide, 50 high)
    im[20:70, w - off - 44:w - off] = DARK              # right
    return im


def border_frames():
    return np.stack([border_frame(2), border_frame(3)])


# ---- long_reversed ---------------------------------------------------------------------------------------------------------------------------
LONG_W, LONG_H = 272, 200
REVERSED_FAMILIES = ["std41r", "std52r"]   # a reversed-only configuration of tests/stress_families.py


def long_frame(bright_on_dark=False, side=160, skew=0.1):
    """One slightly skewed square of `side` px: edges of more than 136 px take more than 16 refinement samples."""
    yy, xx = np.mgrid[0:LONG_H, 0:LONG_W]
    m = (np.abs((xx - LONG_W / 2) - skew * (yy - LONG_H / 2)) < side / 2) & (np.abs(yy - LONG_H / 2) < side / 2)
    fg, bg = (BRIGHT, DARK) if bright_on_dark else (DARK, BRIGHT)
    return np.where(m, fg, bg).astype(np.uint8)


# ---- classes: a quad from a cluster of every thread count k_fit runs at ----------------------------------------------------------------------
# points of a cluster (before duplicate removal) up to -> threads of its workgroup (k_quads.hip: FIT_CLASS; what only a workgroup of
# several waves does — one pair fit per lane, reductions and broadcasts across waves — runs at 128, 256 and 512).  Beyond 16 384 points
# a cluster needs a frame of more than 1 400 px: left to the detect tests.
CLASS_THREADS = ((512, 64), (1024, 128), (4096, 256), (16384, 512))
# sides (px of the quad image) of one slightly skewed dark square per thread count, about 12.15 points per pixel of side: 436, 728,
# 1 460 and 4 102 points in the trace (check_classes returns them).  The last is the smallest side whose outline has more than 4 096
# (336 px: 4 090 points).
CLASS_SIDES = (36, 60, 120, 337)
# One frame, repeated: one more than a call may bring and still run its size classes side by side (k_quads.hip: ck_launch_fit_quads) —
# such a call does without the class of 513..1024 points and would fit them on 256 threads; the batch plan has all four thread counts.
CLASS_FRAMES = {1: 17, 2: 33}


def classes_frame(decimate, sides=CLASS_SIDES, skew=0.1):
    """The largest square as a dark frame 18 px thick (its inner outline, bright inside dark, leaves at the border direction), the
    others dark on its bright inside: the image is no larger than the largest square needs.  Everything scales with quad_decimate,
    so the clusters of the decimated image are those of quad_decimate 1."""
    d, big = decimate, sides[-1]
    h, w = d * (big + 24), d * (int(big * (1 + skew)) + 26)
    yy, xx = np.mgrid[0:h, 0:w]
    inside = lambda cx, cy, s: (np.abs((xx - cx) - skew * (yy - cy)) < d * s / 2) & (np.abs(yy - cy) < d * s / 2)
    im = np.full((h, w), BRIGHT, np.uint8)
    im[inside(w / 2, h / 2, big)] = DARK
    im[inside(w / 2, h / 2, big - 36)] = BRIGHT
    x = w / 2 - d * (big - 36) / 2 + d * 24
    for s in sides[-2::-1]:   # left to right, the largest first, centred on the middle row
        im[inside(x + d * s / 2, h / 2, s)] = DARK
        x += d * (s + 16)
    return im


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
TIES_SEEDS, TIES_NMAXIMA = (4, 6), (9, 10, 11)   # found by search_ties: the frames in which a tie straddles the cut and two subsets tie
BORDER_OFFSETS = (1, 2, 3)
BATCH_FRAMES = 40   # more than the 16 (quad_decimate 1) or 32 (2) frames up to which a call runs its size classes side by side


def search_ties(oracle, seeds=range(12), nmaxima=TIES_NMAXIMA):
    """The search that found TIES_SEEDS: (seed, max_nmaxima, clusters whose cut kept fewer than max_nmaxima, clusters that became a
    quad after two or more 4-subsets had tied for the best energy)."""
    out = []
    for seed in seeds:
        f = symmetric_blobs(seed)
        for m in nmaxima:
            rd, _ = trace(oracle, f, dict(TIES_SETTINGS, max_nmaxima=m))
            out.append((seed, m, int(((rd[:, FOUND] > m) & (rd[:, KEPT] < m)).sum()), int(((rd[:, TIES] >= 2) & (rd[:, EXIT] == QUAD)).sum())))
    return out


def _exits(rd):
    return {int(k): int(v) for k, v in zip(*np.unique(rd[:, EXIT], return_counts=True))}


def _need(figures, minimum):
    """Every figure named in `minimum` is at least that; returns the figures."""
    for k, v in minimum.items():
        assert figures[k] >= v, f"{k} = {figures[k]}, needs >= {v}: {figures}"
    return figures


def check_small(oracle, frames, settings, rd, quads):
    found = rd[:, FOUND]
    fig = {"ksz == 2": int((rd[:, KSZ] == 2).sum()), "24 points after duplicate removal": int((rd[:, UNIQUE] == 24).sum()),
           ">= 24 points before, < 24 after (exit 5)": int(((rd[:, POINTS] >= 24) & (rd[:, UNIQUE] >= 0) & (rd[:, UNIQUE] < 24) & (rd[:, EXIT] == 5)).sum()),
           "exit 6": int((rd[:, EXIT] == 6).sum()), "2 maxima": int((found == 2).sum()), "3 maxima": int((found == 3).sum()),
           "4 maxima": int((found == 4).sum()), "quads": sum(len(q) for q in quads.values())}
    return _need(fig, {"ksz == 2": 5, "24 points after duplicate removal": 1, ">= 24 points before, < 24 after (exit 5)": 1, "exit 6": 1,
                       "2 maxima": 1, "3 maxima": 1, "4 maxima": 1, "quads": 10})


def check_mse(oracle, frames, settings, rd, quads):
    at8 = rd[rd[:, EXIT] == 8]
    return _need({"exit 8": len(at8), "their points": at8[:, UNIQUE].tolist()}, {"exit 8": 1})


def check_noise(oracle, frames, settings, rd, quads):
    m, ex = settings["max_nmaxima"], _exits(rd)
    fig = {"nmax == max_nmaxima": int((rd[:, FOUND] == m).sum()), "nmax == max_nmaxima + 1": int((rd[:, FOUND] == m + 1).sum()),
           "nmax >= 65": int((rd[:, FOUND] >= 65).sum()), "largest nmax": int(rd[:, FOUND].max()), "ksz == 20": int((rd[:, KSZ] == 20).sum()),
           "quads": sum(len(q) for q in quads.values())}
    fig.update({"exit %d" % k: ex.get(k, 0) for k in (7, 10, 11, 12, 13)})
    return _need(fig, dict({"nmax == max_nmaxima": 1, "nmax == max_nmaxima + 1": 1, "nmax >= 65": 1, "ksz == 20": 1, "quads": 5},
                           **{"exit %d" % k: 1 for k in (7, 10, 11, 12, 13)}))


def check_ties(oracle, frames, settings, rd, quads):
    m = settings["max_nmaxima"]
    for f in frames:
        assert np.array_equal(f, f.T)
    over = rd[:, FOUND] > m
    fig = {"more maxima than the cut": int(over.sum()), "of them kept < max_nmaxima (tie across the cut)": int((over & (rd[:, KEPT] < m)).sum()),
           "subsets tied for the best energy": int((rd[:, TIES] >= 2).sum()), "of them quads": int(((rd[:, TIES] >= 2) & (rd[:, EXIT] == QUAD)).sum())}
    return _need(fig, {"of them kept < max_nmaxima (tie across the cut)": 1, "of them quads": 1})


def check_border(oracle, frames, settings, rd, quads):
    """corner distances BEFORE refinement: the same frames with refine_edges = 0"""
    assert settings["refine_edges"] == 1
    h, w = frames[0].shape
    near, dists = 0, []
    for f in frames:
        _, q0 = trace(oracle, f, dict(settings, refine_edges=0))
        for row in q0:
            p = row[:8].reshape(4, 2)
            d = float(np.min([p[:, 0], w - p[:, 0], p[:, 1], h - p[:, 1]]))
            dists.append(round(d, 2))
            near += d < settings["quad_decimate"] + 1
    return _need({"quads with a corner closer than quad_decimate + 1 to the border": int(near), "corner distances": sorted(dists),
                  "quads": sum(len(q) for q in quads.values())}, {"quads with a corner closer than quad_decimate + 1 to the border": 1})


def _longest_edge(quads):
    out = 0.0
    for q in quads.values():
        for row in q:
            p = row[:8].reshape(4, 2)
            out = max(out, float(np.hypot(*(p - np.roll(p, -1, 0)).T).max()))
    return out


def check_long(oracle, frames, settings, rd, quads):
    assert settings["refine_edges"] == 1
    return _need({"longest edge": round(_longest_edge(quads), 1)}, {"longest edge": 136.01})


def check_reversed(oracle, frames, settings, rd, quads):
    assert settings["refine_edges"] == 1
    rev = sum(int((q[:, 8] == 1).sum()) for q in quads.values())
    return _need({"quads with reversed_border": rev, "clusters with reversed": int((rd[:, REVERSED] == 1).sum()),
                  "longest edge": round(_longest_edge(quads), 1)}, {"quads with reversed_border": 1})


def check_batch(oracle, frames, settings, rd, quads):
    assert len(frames) > (16 if settings["quad_decimate"] == 1 else 32)
    return _need({"frames": len(frames), "distinct frames": len(quads), "quads in the distinct frames": sum(len(q) for q in quads.values())},
                 {"quads in the distinct frames": 10})


def quads_per_thread_count(rd):
    """{threads: point counts of the clusters that left as quads} on the readouts, by CLASS_THREADS"""
    q, out, lo = rd[rd[:, EXIT] == QUAD], {}, 0
    for top, nth in CLASS_THREADS:
        out[nth] = q[(q[:, POINTS] > lo) & (q[:, POINTS] <= top), POINTS].tolist()
        lo = top
    return out


def check_classes(oracle, frames, settings, rd, quads):
    """per thread count of k_fit: a cluster that leaves as a quad, with edge refinement on, in a call that takes the batch plan"""
    assert settings["refine_edges"] == 1
    assert len(frames) == CLASS_FRAMES[settings["quad_decimate"]] > (16 if settings["quad_decimate"] == 1 else 32)
    per = quads_per_thread_count(rd)
    fig = {"quads from %d threads" % nth: len(p) for nth, p in per.items()}
    fig.update({"their points (%d threads)" % nth: p for nth, p in per.items()})
    fig["frame"] = frames[0].shape
    return _need(fig, {"quads from %d threads" % nth: 1 for _, nth in CLASS_THREADS})


def _batch_frames():
    one = np.concatenate([small_frames(), noise_frames()])
    return np.concatenate([one] * (BATCH_FRAMES // len(one)))


def _noise_name(s):
    return "noise_m%d_d%d_r%d" % (s["max_nmaxima"], s["quad_decimate"], s["refine_edges"]) + ("_cos0.5" if "cos_critical_rad" in s else "")


def specs():
    """[(name, function that draws the frames, settings, check)] of every case; check(oracle, frames, settings, readouts, quads)
    asserts the case's conditions and returns the figures it measured."""
    out = [("small", small_frames, dict(SMALL_SETTINGS), check_small)]
    for k, (v, which) in enumerate(MSE_WINDOW):
        out.append(("mse_window_%d" % k, (lambda which=which: small_frames()[list(which)]), dict(SMALL_SETTINGS, max_line_fit_mse=v), check_mse))
    out += [(_noise_name(s), noise_frames, dict(s), check_noise) for s in NOISE_SETTINGS]
    ties = lambda: np.stack([symmetric_blobs(s) for s in TIES_SEEDS])
    out += [("ties_m%d" % m, ties, dict(TIES_SETTINGS, max_nmaxima=m), check_ties) for m in TIES_NMAXIMA]
    border = lambda: np.stack([border_frame(o) for o in BORDER_OFFSETS])
    out += [("border_d%d" % d, border, {"quad_decimate": d, "refine_edges": 1}, check_border) for d in (1, 2)]
    out.append(("long", lambda: long_frame()[None], {"refine_edges": 1}, check_long))
    out.append(("reversed", lambda: long_frame(bright_on_dark=True)[None], {"refine_edges": 1, "families": list(REVERSED_FAMILIES)}, check_reversed))
    out += [("batch_d%d" % d, _batch_frames, {"quad_decimate": d}, check_batch) for d in (1, 2)]
    out += [("classes_d%d" % d, (lambda d=d: np.stack([classes_frame(d)] * CLASS_FRAMES[d])), {"quad_decimate": d, "refine_edges": 1}, check_classes)
            for d in (1, 2)]
    return out


NAMES = [s[0] for s in specs()]
_built = {}


def case(name):
    """(frames, settings, check) of the named case; the frames are drawn once per process."""
    if name not in _built:
        _, draw, settings, check = next(s for s in specs() if s[0] == name)
        _built[name] = (np.ascontiguousarray(draw(), np.uint8), settings, check)
    return _built[name]


def measure(oracle, name):
    """(figures, {frame: sorted quads} of the distinct frames, index, readouts): the oracle's trace of the case, its conditions asserted."""
    frames, settings, check = case(name)
    rd, quads, index = case_trace(oracle, frames, settings)
    assert not (rd[:, EXIT] == 9).any(), "exit 9 repeats line fits that have passed: no case reaches it"
    return check(oracle, frames, settings, rd, quads), quads, index, rd
