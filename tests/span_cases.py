"""Inputs of the parity test of the split quad fit's middle kernel at every alignment to its grid (tests/test_gpu_span_alignment.py;
tests/test_span_cases_host.py proves on the CPU that the cases reach what they name).  Nothing here touches the GPU.

k_chunk and k_tail (chalkydri_amd/csrc/k_quads.hip) are written around a fixed grid of positions — spans of CK_SPAN = 960, words of
64, blocks of 32 — while a cluster's place on it is handed out by an atomic counter in the order the clusters get to k_seq's step 4.
The diagnostics build's CK_EXT_BASE sets the first position handed out in every frame of a call; in a frame in which exactly ONE
cluster reaches step 4, that cluster's extended sequence then starts at es = base, its points lie at [e0, e1) = [base + CK_EXT_PRE,
base + CK_EXT_PRE + sz), and the frame's live positions end at es + sz + CK_EXT_HALO.  The sweep frames below are such frames: a
dark square on a bright sheet, one cluster, which becomes a quad, so a wrong maximum, rank or prefix sum at any placement changes or
loses that quad.  Their sizes after duplicate removal (sz), window half-widths and numbers of maxima were traced on the oracle and
are pinned; CONDITIONS re-assert them.  placement() names the grid's edges that (sz, maxima, base) meets.

The crowded frames are for k_chunk's loop over several spans per workgroup (the next span's points and weights fetched while this
one is worked on): enough live positions per frame that each of the 8 workgroups a frame gets at least takes two spans."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import quad_cases as qc
import tail_selection_cases as tc
from quad_cases import EXIT, FOUND, KSZ, QUAD, UNIQUE

SPAN = 960                       # CK_SPAN of ck_internal.h
EXT_PRE, EXT_POST = 25, 24       # CK_EXT_PRE, CK_EXT_POST of ck_internal.h
HALO = EXT_PRE + EXT_POST
KOFF = 32                        # k_chunk.hip: positions k_chunk loads in front of the span it decides
SHEET, BIG_SHEET = tc.SHEET, tc.BIG_SHEET
BASES = range(1024)              # every residue of e0, e1 and of every maximum modulo 960, the cluster starting in span 0 and in span 1
BASE_MAX = 2 * SPAN              # the library clamps CK_EXT_BASE to this
POISON_BASES = list(range(128)) + list(range(896, 1024))   # the placements around span 0's start and around the first span boundary
LOOP_BASES = (0, 1, 31, 935, 959, 960)
LOOP_WGS = 8                     # k_chunk's workgroups per frame under CK_CHUNK_WGS=0 (the grid's minimum)
SMALL_AT = 144                   # where the 64 x 64 sheet of a small square lies on the 352 sheet


def small_square(half, cx, cy, angle, sheet=SHEET):
    """One hard-edged dark square of half-size `half` px, turned by `angle` about (cx, cy) of a 64 x 64 patch in the middle of a
    bright sheet: a pixel is dark when its centre lies inside (quad_cases.small_sheet's rule)."""
    y, x = np.mgrid[0:64, 0:64] + 0.5
    ca, sa = math.cos(angle), math.sin(angle)
    m = (np.abs((x - cx) * ca + (y - cy) * sa) < half) & (np.abs(-(x - cx) * sa + (y - cy) * ca) < half)
    im = np.full((sheet, sheet), tc.BRIGHT, np.uint8)
    im[SMALL_AT:SMALL_AT + 64, SMALL_AT:SMALL_AT + 64][m] = tc.DARK
    return im


# (half, cx, cy, angle) of the small squares, found by search_small: the window half-width travels in the point word, ksz = sz / 12 < 20
# below 240 points
SMALL = {64: (3.84, 32.122, 32.23, 0.015), 120: (6.9, 32.45, 31.644, 1.49), 232: (10.36, 32.164, 31.661, 0.694), 240: (10.6, 32.096, 32.186, 0.691)}


def search_small(oracle, tries=6000, seed=1):
    """The search that found SMALL: {sz: (half, cx, cy, angle, ksz, maxima)} of the frames whose only cluster at the fit becomes a quad."""
    rng, out = np.random.default_rng(seed), {}
    for _ in range(tries):
        half, cx, cy = round(float(rng.uniform(2.6, 11.0)), 2), round(32 + float(rng.uniform(-0.5, 0.5)), 3), round(32 + float(rng.uniform(-0.5, 0.5)), 3)
        ang = round(float(rng.uniform(0, np.pi / 2)), 3)
        rd, q = qc.trace(oracle, small_square(half, cx, cy, ang), {})
        live = rd[rd[:, EXIT] >= 6]
        if len(live) == 1 and live[0, EXIT] == QUAD and len(q) == 1:
            out.setdefault(int(live[0, UNIQUE]), (half, cx, cy, ang, int(live[0, KSZ]), int(live[0, FOUND])))
    return out


def _clean(side):
    return lambda: tc.noisy_square(0, SHEET, float(side), amp=0)


def _edge(k):
    side, seed, _ = tc.EDGES[k]
    return lambda: tc.noisy_square(seed, SHEET, side)


# (name, sheet, function that draws the frame, points after duplicate removal, ksz, maxima): as traced on the oracle, default settings
SWEEP = [("small_%d" % sz, SHEET, (lambda p=p: small_square(*p)), sz, ksz, found)
         for (sz, p), (ksz, found) in zip(sorted(SMALL.items()), ((5, 4), (10, 7), (19, 11), (20, 14)))]
SWEEP += [("clean_%d" % side, SHEET, _clean(side), sz, 20, found)
          for side, sz, found in ((40, 336, 12), (80, 672, 28), (120, 1008, 46), (160, 1344, 64), (240, 2016, 100), (300, 2520, 126))]
SWEEP += [("edge_%d" % found, SHEET, _edge(k), sz, 20, found) for k, (sz, found) in enumerate(((808, 64), (792, 65), (2520, 256), (2560, 257)))]
SWEEP += [("beyond", BIG_SHEET, (lambda: tc.noisy_square(tc.BEYOND[1], BIG_SHEET, tc.BEYOND[0])), 3360, 20, 322)]
SHEETS = (SHEET, BIG_SHEET)

# what the sizes and the numbers of maxima have to cover: (name, condition on sz) / (name, condition on the maxima)
SIZE_GROUPS = (("one or two spans", lambda sz: sz <= SPAN - HALO), ("two or three spans", lambda sz: SPAN <= sz <= 2 * SPAN - HALO),
               ("three spans or more", lambda sz: sz >= 2 * SPAN + 2), ("four spans or more", lambda sz: sz >= 3 * SPAN))
FOUND_GROUPS = (("one maximum per lane", lambda n: n <= 64), ("maxima in registers", lambda n: 64 < n <= 64 * tc.RV), ("maxima re-read", lambda n: n > 64 * tc.RV))


def sweep_rows(sheet):
    return [r for r in SWEEP if r[1] == sheet]


_frames = {}


def sweep_frames(sheet):
    """[n][sheet][sheet]: the sweep frames of one handle, drawn once per process"""
    if sheet not in _frames:
        _frames[sheet] = np.ascontiguousarray(np.stack([r[2]() for r in sweep_rows(sheet)]), np.uint8)
    return _frames[sheet]


# ---- where a placement lies on the grid ------------------------------------------------------------------------------------------------
def placement(sz, found, base):
    """The edges of k_chunk's and k_tail's grid that the only cluster of a frame meets when the frame's positions start at `base`:
    a set of names.  es: first position of the extended sequence; [e0, e1): the cluster's points; end: the frame's live positions."""
    es = base
    e0, e1, end = es + EXT_PRE, es + EXT_PRE + sz, es + sz + HALO
    nruns = (e1 - 1) // SPAN - e0 // SPAN + 1
    out = {"spans touched: %d" % nruns, "heads prefetch" if nruns <= 2 and found <= 64 else "run tables"}
    if e0 % 32 == 0:
        out.add("e0 % 32 == 0")          # phase 5b: the head range [B0 << 5, e0 - 1] is empty
    for r in (0, 1, SPAN - 1):
        if e0 % SPAN == r:
            out.add("e0 %% 960 == %d" % r)   # rank_excl's x == s * CK_SPAN; the first point decided by the span before / as a span's last
    if es == 0:
        out.add("es == 0")               # span 0 loads zeros in front of the sequence
    for r in (0, 1):
        if e1 % SPAN == r:
            out.add("e1 %% 960 == %d" % r)   # the last point is a span's last / a span's first
        if end % SPAN == r:
            out.add("end %% 960 == %d" % r)  # the last live span is cut at the sequence's end / holds one position
    return out


def edges_possible(sz, found):
    """Every edge that some base of BASES reaches for a cluster of sz points and `found` maxima."""
    out = set()
    for b in BASES:
        out |= placement(sz, found, b)
    return out


GRID_EDGES = ("e0 % 32 == 0", "e0 % 960 == 0", "e0 % 960 == 1", "e0 % 960 == 959", "es == 0", "e1 % 960 == 0", "e1 % 960 == 1",
              "end % 960 == 0", "end % 960 == 1")


def edges_required(group):
    """What the bases have to reach for at least one frame of the size group: every grid edge, both numbers of spans a cluster of the
    group can touch, and the ways k_tail gets at the maxima that the group allows (up to two runs: prefetched by the heads or not,
    by the number of maxima; three runs and more: the run tables)."""
    lo = {"one or two spans": 1, "two or three spans": 2, "three spans or more": 3, "four spans or more": 4}[group]
    ways = {"one or two spans": {"heads prefetch", "run tables"}, "two or three spans": {"heads prefetch", "run tables"}}.get(group, {"run tables"})
    return set(GRID_EDGES) | {"spans touched: %d" % lo, "spans touched: %d" % (lo + 1)} | ways


# ---- the crowded frames ----------------------------------------------------------------------------------------------------------------
CROWDED_W, CROWDED_H = 640, 480
CROWDED_MIN = 2 * LOOP_WGS * SPAN   # live positions above which each of the 8 workgroups takes at least two spans and some take three


def _H(cx, cy, side, deg):
    a, c, s = side / 2.0, math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [[a * c, -a * s, cx], [a * s, a * c, cy], [0.0, 0.0, 1.0]]


def crowded_frames():
    """Two frames of 640x480 with eight tags of side 50-160 px on the bench's background (ramp, noise +-3): the noise supplies the
    clusters that fill the spans."""
    from chalkydri_amd import synth
    lay = [(110, 110, 160), (90, 370, 110), (250, 400, 80), (330, 90, 100), (490, 70, 70), (560, 210, 90), (410, 320, 130), (580, 410, 50)]
    frames = []
    for i in range(2):
        tags = [(0, 20 * i + k, _H(cx + 3 * i, cy + i, side, 5 * i - 4 + (k & 1))) for k, (cx, cy, side) in enumerate(lay)]
        frames.append(synth.render_scene(700 + i, CROWDED_W, CROWDED_H, tags, noise_amp=3)[0])
    return np.ascontiguousarray(np.stack(frames), np.uint8)


# ---- conditions, on the oracle's per-cluster readout -----------------------------------------------------------------------------------
def check_sweep(oracle):
    """(figures, {sheet: [sorted quads per frame]}): every sweep frame traced once; no case is dropped, one that stops meeting its
    condition fails with the figure."""
    fig, quads = {}, {s: [] for s in SHEETS}
    for sheet in SHEETS:
        for (name, _, _, sz, ksz, found), f in zip(sweep_rows(sheet), sweep_frames(sheet)):
            rd, q = qc.trace(oracle, f, {})
            live = rd[rd[:, EXIT] >= 6]
            assert len(live) == 1 and live[0, EXIT] == QUAD and len(q) == 1, "%s: clusters at the fit %s, quads %d" % (name, live.tolist(), len(q))
            got = (int(live[0, UNIQUE]), int(live[0, KSZ]), int(live[0, FOUND]))
            assert got == (sz, ksz, found), "%s: (points, ksz, maxima) = %s, pinned %s" % (name, got, (sz, ksz, found))
            fig[name] = got
            quads[sheet].append(q)
    for gname, cond in SIZE_GROUPS:
        fig["sizes, " + gname] = [r[3] for r in SWEEP if cond(r[3])]
        assert fig["sizes, " + gname], gname
    for gname, cond in FOUND_GROUPS:
        fig["maxima, " + gname] = [r[5] for r in SWEEP if cond(r[5])]
        assert fig["maxima, " + gname], gname
    fig["ksz"] = sorted(set(r[4] for r in SWEEP))
    assert min(fig["ksz"]) < 20 and fig["ksz"][-1] == 20 and 19 in fig["ksz"], fig["ksz"]
    return fig, quads


def check_crowded(oracle):
    """(figures, [sorted quads per frame]): the live positions of each crowded frame, from the clusters that reach the fit"""
    frames = crowded_frames()
    assert frames.shape == (2, CROWDED_H, CROWDED_W)
    fig, quads = {}, []
    for i, f in enumerate(frames):
        rd, q = qc.trace(oracle, f, {})
        live = rd[rd[:, EXIT] >= 6]
        pos = int((live[:, UNIQUE] + HALO).sum())
        fig["frame %d" % i] = {"clusters at the fit": len(live), "live positions": pos, "spans": -(-pos // SPAN), "quads": len(q)}
        assert pos > CROWDED_MIN, "frame %d: %d live positions, needs > %d" % (i, pos, CROWDED_MIN)
        assert len(q) >= 8, "frame %d: %d quads, the eight tags' are among the oracle's" % (i, len(q))
        quads.append(q)
    return fig, quads


CONDITIONS = {"sweep": check_sweep, "crowded": check_crowded}
