"""The iterative tri-class Otsu threshold of DESIGN.md §4h, twice.

solve()        the contract restated operation for operation in plain Python integers and Python floats: what ck_tri_otsu_solve
               and k_tri_solve must reproduce byte for byte (record and table).
solve_exact()  an independent solver in fractions.Fraction: exact v(t), an exact arg-max, and the classes decided level by level by
               comparing each gray value with the rational class means round by round: no interval arithmetic, no ceil / floor, no
               table.  It also reports the smallest relative gap between the best and the next different v of any round, so a test
               can tell a disagreement that fp64 rounding may cause (a near-tie) from one that it may not.
gray() / histogram() / classify()   the CAT gray map (utils.rs:33-46) vectorised, and a frame through solve().
"""
from fractions import Fraction

import numpy as np

MAX_ROUNDS, FLAT = 32, 1
INFO_DTYPE = np.dtype([("n_rounds", "<i4"), ("T", "<i4", (MAX_ROUNDS,)), ("T_last", "<i4"), ("lo_final", "<i4"), ("hi_final", "<i4"),
                       ("n_black", "<u4"), ("n_white", "<u4"), ("n_other", "<u4"), ("flags", "<u4")])
BLACK, WHITE, OTHER = 0, 1, 2


def gray(r, g, b):
    """trunc(fma(r, 0.33f, fma(g, 0.33f, b * 0.33f))) in f32, saturated to 0..255, on uint8 arrays.  A product of an 8-bit and a
    24-bit number plus a 24-bit number of similar size is exact in f64, so rounding that sum to f32 is the fma's single rounding."""
    k = np.float32(0.33)
    r, g, b = (np.asarray(v).astype(np.float32) for v in (r, g, b))
    inner = (g.astype(np.float64) * np.float64(k) + (b * k).astype(np.float64)).astype(np.float32)
    outer = (r.astype(np.float64) * np.float64(k) + inner.astype(np.float64)).astype(np.float32)
    return np.clip(np.trunc(outer), 0, 255).astype(np.uint8)


def gray_frame(frame):
    """[h][w][3] -> gray(r, g, b); [h][w] or [h][w][1] -> gray(v, v, v)."""
    frame = np.asarray(frame, np.uint8)
    if frame.ndim == 3 and frame.shape[2] == 3:
        return gray(frame[..., 0], frame[..., 1], frame[..., 2])
    v = frame.reshape(frame.shape[0], frame.shape[1])
    return gray(v, v, v)


def histogram(g):
    return np.bincount(np.asarray(g, np.uint8).reshape(-1), minlength=256).astype(np.uint32)


def _wrap64(x):
    """a Python integer as the int64 of 64-bit two's complement arithmetic (the identity while |x| < 2^63)"""
    return ((x + (1 << 63)) % (1 << 64)) - (1 << 63)


def solve(hist, max_iters=8, min_delta=1, keep_tbd=1):
    """-> (record as a numpy scalar of INFO_DTYPE, lut uint8[256])"""
    hist = [int(v) for v in np.asarray(hist).reshape(-1)]
    assert len(hist) == 256 and 1 <= max_iters <= MAX_ROUNDS and 1 <= min_delta <= 255 and keep_tbd in (0, 1)
    info = np.zeros((), INFO_DTYPE)
    info["T"][:] = -1
    lo, hi, T_last, rounds = 0, 255, -1, 0
    k = 0
    while True:
        k += 1
        N = S = occupied = 0
        for g in range(lo, hi + 1):
            if hist[g]:
                N += hist[g]
                S += g * hist[g]
                occupied += 1
        if occupied < 2:
            break
        n = s = 0
        best, T, n_T, s_T = -1.0, -1, 0, 0
        for t in range(lo, hi):
            n += hist[t]
            s += t * hist[t]
            if n > 0 and N - n > 0:
                d = float(_wrap64(S * n - N * s))
                v = (d * d) / (float(n) * float(N - n))
                if v > best:
                    best, T, n_T, s_T = v, t, n, s
        lo2 = (s_T + n_T - 1) // n_T           # ceil of the lower class mean
        hi2 = (S - s_T) // (N - n_T)           # floor of the upper class mean
        repeat = k >= 2 and abs(T - T_last) < min_delta
        info["T"][k - 1] = T
        T_last, rounds = T, k
        if repeat or k == max_iters:
            lo, hi = lo2, hi2
            break
        if lo2 > hi2:
            break
        lo, hi = lo2, hi2
    info["n_rounds"], info["T_last"], info["lo_final"], info["hi_final"] = rounds, T_last, lo, hi
    info["flags"] = FLAT if rounds == 0 else 0
    lut = np.zeros(256, np.uint8)
    counts = [0, 0, 0]
    for g in range(256):
        if rounds == 0:
            c = BLACK if g < 128 else WHITE
        elif g < lo:
            c = BLACK
        elif g > hi:
            c = WHITE
        else:
            c = OTHER if keep_tbd else (BLACK if g <= T_last else WHITE)
        lut[g] = c
        counts[c] += hist[g]
    info["n_black"], info["n_white"], info["n_other"] = (v % (1 << 32) for v in counts)
    return info, lut


def solve_exact(hist, max_iters=8, min_delta=1, keep_tbd=1):
    """-> dict(T=[...], lut=uint8[256], lo=, hi=, min_gap=Fraction or None).  State: the decision of every gray level."""
    hist = [int(v) for v in np.asarray(hist).reshape(-1)]
    state = [None] * 256                       # None = to be determined
    Ts, min_gap = [], None
    while True:
        tbd = [g for g in range(256) if state[g] is None]
        if sum(1 for g in tbd if hist[g]) < 2:
            break
        N, S = sum(hist[g] for g in tbd), sum(g * hist[g] for g in tbd)
        cands = []                             # (v, t, n, s)
        n = s = 0
        for t in tbd[:-1]:
            n += hist[t]
            s += t * hist[t]
            if n > 0 and N - n > 0:
                cands.append((Fraction((S * n - N * s) ** 2, n * (N - n)), t, n, s))
        vmax = max(c[0] for c in cands)
        _, T, n_T, s_T = min((c for c in cands if c[0] == vmax), key=lambda c: c[1])
        others = [c[0] for c in cands if c[0] != vmax]
        if others and vmax > 0:
            gap = (vmax - max(others)) / vmax
            min_gap = gap if min_gap is None else min(min_gap, gap)
        mu0, mu1 = Fraction(s_T, n_T), Fraction(S - s_T, N - n_T)
        decided = {g: (BLACK if g < mu0 else WHITE) for g in tbd if g < mu0 or g > mu1}
        k = len(Ts) + 1
        repeat = k >= 2 and abs(T - Ts[-1]) < min_delta
        Ts.append(T)
        if len(decided) == len(tbd) and not (repeat or k == max_iters):
            break                              # nothing would be left to determine: the new region is not adopted
        for g, c in decided.items():
            state[g] = c
        if repeat or k == max_iters:
            break
    tbd = [g for g in range(256) if state[g] is None]
    lut = np.zeros(256, np.uint8)
    for g in range(256):
        if not Ts:
            lut[g] = BLACK if g < 128 else WHITE
        elif state[g] is not None:
            lut[g] = state[g]
        else:
            lut[g] = OTHER if keep_tbd else (BLACK if g <= Ts[-1] else WHITE)
    return {"T": Ts, "lut": lut, "lo": tbd[0] if tbd else None, "hi": tbd[-1] if tbd else None, "min_gap": min_gap}


def classify(frame, **params):
    """A frame through the restatement: (classes [h][w], record, hist)."""
    g = gray_frame(frame)
    hist = histogram(g)
    info, lut = solve(hist, **params)
    return lut[g], info, hist
