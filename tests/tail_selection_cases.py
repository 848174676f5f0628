"""Inputs of the parity test of the tail's rank selection (tests/test_gpu_tail_selection.py; tests/test_tail_selection_cases_host.py
proves on the CPU that the cases reach what they name).  Nothing here touches the GPU.

k_tail (chalkydri_amd/csrc/k_quads.hip, k_tail_body 5a) cuts a cluster's maxima to the max_nmaxima strongest in one of three ways: up
to 64 maxima one per lane, up to 64 * RV held in registers RV per lane, beyond that by re-reading them round by round.  The cases
put clusters at the sizes where the way changes, a tie across the cut on the register path, and a cluster in three or more spans of
960 positions on it, all of them clusters that BECOME quads: a wrong survivor changes or loses a quad.  One dark square on a bright
sheet under noise of +-2 is one cluster (the flat parts stay below min_white_black_diff); its number of maxima follows its side and
the noise, so the sides and seeds below were searched (search_edges, search_ties) and are pinned; CONDITIONS re-assert on the oracle's
per-cluster readout what each case is for."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import quad_cases as qc
from quad_cases import EXIT, FOUND, KEPT, QUAD, UNIQUE

RV = 4                       # SEL_RV of k_quads.hip
SPAN = 960                   # CK_SPAN of ck_internal.h
THREE_SPANS = 2 * SPAN + 2   # points that touch three spans wherever the cluster starts
BRIGHT, DARK = 215, 40
SHEET, BIG_SHEET = 352, 448


def noisy_square(seed, sheet, side, amp=2, symmetric=False, skew=0.1):
    """One dark square of `side` px on a bright sheet under noise of +-amp.  Skewed by `skew` and off centre by up to 2 px; or
    (symmetric) axis-aligned and centred, under noise mirrored in the main diagonal: the frame equals its transpose, so its
    maxima come in mirrored pairs whose smoothed errors are often equal to the bit."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:sheet, 0:sheet].astype(np.float64)
    if symmetric:
        m = (np.abs(xx - sheet / 2) < side / 2) & (np.abs(yy - sheet / 2) < side / 2)
    else:
        cx, cy = sheet / 2 + rng.uniform(-2, 2), sheet / 2 + rng.uniform(-2, 2)
        m = (np.abs((xx - cx) - skew * (yy - cy)) < side / 2) & (np.abs(yy - cy) < side / 2)
    im = np.where(m, DARK, BRIGHT).astype(np.int64)
    nz = rng.integers(-amp, amp + 1, (sheet, sheet))
    if symmetric:
        nz = np.triu(nz)
        nz = nz + np.triu(nz, 1).T
    return np.clip(im + nz, 0, 255).astype(np.uint8)


# (side, seed, maxima of the square's cluster): the last cluster of the one-per-lane path and the first of the register path, the
# last of the register path and the first beyond it
EDGES = [(96.0, 0, 64), (94.0, 43, 65), (300.0, 0, 64 * RV), (305.0, 14, 64 * RV + 1)]
BUSY = (160.0, 0)            # (side, seed) under noise of +-3: the flat parts break up into a hundred-odd clusters around the square
BEYOND = (400.0, 0)          # (side, seed) on the big sheet: well beyond 64 * RV maxima
TIES_SIDE, TIES_SEEDS, TIES_NMAXIMA = 200.0, (25, 33, 35), (10, 12)   # (no tie straddles a cut of 4 in seeds 0 .. 249: the four strongest are the corners)
NMAXIMA = (4, 10, 12)


def edge_frames():
    return np.stack([noisy_square(seed, SHEET, side) for side, seed, _ in EDGES] + [noisy_square(BUSY[1], SHEET, BUSY[0], amp=3)])


def beyond_frames():
    return noisy_square(BEYOND[1], BIG_SHEET, BEYOND[0])[None]


def ties_frames():
    return np.stack([noisy_square(s, SHEET, TIES_SIDE, symmetric=True) for s in TIES_SEEDS])


def search_edges(oracle, sides, seeds=range(150), sheet=SHEET):
    """The search that found EDGES: {maxima: (side, seed)} of the frames whose only cluster becomes a quad."""
    out = {}
    for side in sides:
        for seed in seeds:
            rd, _ = qc.trace(oracle, noisy_square(seed, sheet, side), {})
            if len(rd) == 1 and rd[0, EXIT] == QUAD:
                out.setdefault(int(rd[0, FOUND]), (side, seed))
    return out


def search_ties(oracle, side=TIES_SIDE, seeds=range(40), nmaxima=NMAXIMA):
    """The search that found TIES_SEEDS: (seed, max_nmaxima, maxima, kept) wherever a tie straddles the cut of a cluster of more than 64."""
    out = []
    for seed in seeds:
        for m in nmaxima:
            rd, _ = qc.trace(oracle, noisy_square(seed, SHEET, side, symmetric=True), {"max_nmaxima": m})
            out += [(seed, m, int(r[FOUND]), int(r[KEPT])) for r in rd if r[FOUND] > 64 and r[KEPT] < m]
    return out


def check_edges(oracle, frames, settings, rd, quads):
    m = settings["max_nmaxima"]
    quad = rd[:, EXIT] == QUAD
    fig = {"quads of %d maxima" % n: int((quad & (rd[:, FOUND] == n)).sum()) for _, _, n in EDGES}
    on_regs = (rd[:, FOUND] > 64) & (rd[:, FOUND] <= 64 * RV)
    fig.update({"clusters of 65 .. %d maxima" % (64 * RV): int(on_regs.sum()), "of them cut to max_nmaxima": int((on_regs & (rd[:, KEPT] == m)).sum()),
                "of them in three or more spans": int((on_regs & (rd[:, UNIQUE] >= THREE_SPANS)).sum()),
                "of them in three or more spans, quads": int((on_regs & quad & (rd[:, UNIQUE] >= THREE_SPANS)).sum()),
                "clusters of at most 64 maxima and more than max_nmaxima": int(((rd[:, FOUND] <= 64) & (rd[:, FOUND] > m)).sum()),
                "clusters": len(rd), "quads": sum(len(q) for q in quads.values())})
    need = {k: 1 for k in fig if k.startswith("quads of")}
    need.update({"clusters of 65 .. %d maxima" % (64 * RV): 10, "of them cut to max_nmaxima": 10, "of them in three or more spans, quads": 1,
                 "clusters of at most 64 maxima and more than max_nmaxima": 10, "quads": 5})
    return qc._need(fig, need)


def check_beyond(oracle, frames, settings, rd, quads):
    far = rd[:, FOUND] >= 64 * RV + 40
    return qc._need({"clusters well beyond %d maxima" % (64 * RV): int(far.sum()), "of them quads": int((far & (rd[:, EXIT] == QUAD)).sum()),
                     "largest nmax": int(rd[:, FOUND].max())}, {"of them quads": 1})


def check_ties(oracle, frames, settings, rd, quads):
    m = settings["max_nmaxima"]
    for f in frames:
        assert np.array_equal(f, f.T)
    on_regs = (rd[:, FOUND] > 64) & (rd[:, FOUND] <= 64 * RV)
    tie = on_regs & (rd[:, KEPT] < m)
    return qc._need({"clusters of 65 .. %d maxima" % (64 * RV): int(on_regs.sum()), "of them kept < max_nmaxima (tie across the cut)": int(tie.sum()),
                     "of them quads": int((tie & (rd[:, EXIT] == QUAD)).sum()), "kept": rd[tie][:, KEPT].tolist()}, {"of them quads": 1})


def specs():
    """[(name, function that draws the frames, settings, check)], as quad_cases.specs()"""
    out = [("edges_m%d" % m, edge_frames, {"max_nmaxima": m}, check_edges) for m in NMAXIMA]
    out.append(("beyond_m10", beyond_frames, {"max_nmaxima": 10}, check_beyond))
    out += [("ties_m%d" % m, ties_frames, {"max_nmaxima": m}, check_ties) for m in TIES_NMAXIMA]
    return out


NAMES = [s[0] for s in specs()]
_built = {}


def case(name):
    if name not in _built:
        _, draw, settings, check = next(s for s in specs() if s[0] == name)
        _built[name] = (np.ascontiguousarray(draw(), np.uint8), settings, check)
    return _built[name]


def measure(oracle, name):
    """(figures, {frame: sorted quads} of the distinct frames, index, readouts): the oracle's trace of the case, its conditions asserted."""
    frames, settings, check = case(name)
    rd, quads, index = qc.case_trace(oracle, frames, settings)
    return check(oracle, frames, settings, rd, quads), quads, index, rd
