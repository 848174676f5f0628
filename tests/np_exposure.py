"""numpy restatement of the exposure meter: the tables, the statistics of a frame, the metric, the best gamma and
the recommendation.

`stats` is the vectorised form the GPU tests compare against byte for byte; `stats_loops` is written line by line from the
contract with plain loops, and tests/test_exposure_host.py checks that the two agree.  The host arithmetic (metric, recommend)
uses Python floats and math.log / math.exp / math.pow: the same double operations in the same order as ck_exposure_host.c."""
import math

import numpy as np

GAMMAS, BINS = 7, 192
DEFAULT_GAMMAS = (1.0 / 1.9, 1.0 / 1.5, 1.0 / 1.2, 1.0, 1.2, 1.5, 1.9)
STATS_DTYPE = np.dtype([("luma", "<u4", (256,)), ("grad", "<u4", (GAMMAS, BINS)), ("n_luma", "<u4"), ("n_grad", "<u4"), ("pad", "<u4", (2,))])


class Params:
    def __init__(self, gamma=DEFAULT_GAMMAS, lam=1000.0, delta=0.06, kp=1.0, e_min=1e-6, e_max=1e6):
        self.gamma, self.lam, self.delta, self.kp, self.e_min, self.e_max = tuple(float(g) for g in gamma), lam, delta, kp, e_min, e_max


def lut_real(gammas=DEFAULT_GAMMAS):
    """255 (v / 255)^gamma before rounding, [7][256]."""
    return np.array([[255.0 * math.pow(v / 255.0, g) for v in range(256)] for g in gammas])


def luts(gammas=DEFAULT_GAMMAS):
    real = lut_real(gammas)
    out = np.floor(real + 0.5).clip(0, 255).astype(np.uint8)
    out[:, 0], out[:, 255] = 0, 255
    for k, g in enumerate(gammas):
        if g == 1.0:
            out[k] = np.arange(256)
    return out


def clamp_roi(roi, w, h):
    if roi is None:
        return 0, 0, w, h
    x0, y0, x1, y1 = (int(v) for v in roi)
    c = lambda v, hi: min(max(v, 0), hi)
    return c(x0, w), c(y0, h), c(x1, w), c(y1, h)


def isqrt_bins(s):
    """floor(sqrt(s)) >> 3 of an integer array, exact."""
    r = np.floor(np.sqrt(s.astype(np.float64))).astype(np.int64)
    r -= (r * r > s)
    r += ((r + 1) * (r + 1) <= s)
    return r >> 3


def stats(frame, lut, roi=None):
    """One ck_exposure_stats_t (a STATS_DTYPE scalar) of a [h][w] uint8 frame."""
    f = np.asarray(frame, np.uint8)
    h, w = f.shape
    x0, y0, x1, y1 = clamp_roi(roi, w, h)
    out = np.zeros((), STATS_DTYPE)
    if x0 >= x1 or y0 >= y1:
        return out
    out["luma"] = np.bincount(f[y0:y1, x0:x1].reshape(-1), minlength=256)
    out["n_luma"] = (x1 - x0) * (y1 - y0)
    gx0, gy0, gx1, gy1 = max(x0, 1), max(y0, 1), min(x1, w - 1), min(y1, h - 1)
    if gx0 >= gx1 or gy0 >= gy1:
        return out
    out["n_grad"] = (gx1 - gx0) * (gy1 - gy0)
    for k in range(GAMMAS):
        I = lut[k][f].astype(np.int64)
        gx = (I[:-2, 2:] + 2 * I[1:-1, 2:] + I[2:, 2:]) - (I[:-2, :-2] + 2 * I[1:-1, :-2] + I[2:, :-2])
        gy = (I[2:, :-2] + 2 * I[2:, 1:-1] + I[2:, 2:]) - (I[:-2, :-2] + 2 * I[:-2, 1:-1] + I[:-2, 2:])
        b = isqrt_bins(gx * gx + gy * gy)                  # b[y - 1][x - 1] for the pixel (x, y)
        out["grad"][k] = np.bincount(b[gy0 - 1:gy1 - 1, gx0 - 1:gx1 - 1].reshape(-1), minlength=BINS)
    return out


def stats_loops(frame, lut, roi=None):
    """The same, one pixel at a time, as the contract states it."""
    f = [[int(v) for v in row] for row in np.asarray(frame, np.uint8)]
    h, w = len(f), len(f[0])
    x0, y0, x1, y1 = clamp_roi(roi, w, h)
    luma, grad, n_luma, n_grad = [0] * 256, [[0] * BINS for _ in range(GAMMAS)], 0, 0
    for y in range(y0, y1):
        for x in range(x0, x1):
            luma[f[y][x]] += 1
            n_luma += 1
    for y in range(max(y0, 1), min(y1, h - 1)):
        for x in range(max(x0, 1), min(x1, w - 1)):
            n_grad += 1
            for k in range(GAMMAS):
                I = lambda yy, xx: int(lut[k][f[yy][xx]])
                gx = (I(y - 1, x + 1) + 2 * I(y, x + 1) + I(y + 1, x + 1)) - (I(y - 1, x - 1) + 2 * I(y, x - 1) + I(y + 1, x - 1))
                gy = (I(y + 1, x - 1) + 2 * I(y + 1, x) + I(y + 1, x + 1)) - (I(y - 1, x - 1) + 2 * I(y - 1, x) + I(y - 1, x + 1))
                grad[k][math.isqrt(gx * gx + gy * gy) >> 3] += 1
    out = np.zeros((), STATS_DTYPE)
    out["luma"], out["grad"], out["n_luma"], out["n_grad"] = luma, grad, n_luma, n_grad
    return out


def weight(p):
    norm = math.log(p.lam * (1.0 - p.delta) + 1.0)
    return [math.log(p.lam * (b / 180.0 - p.delta) + 1.0) / norm if b / 180.0 >= p.delta else 0.0 for b in range(BINS)]


def metric(p, s):
    W = weight(p)
    n = int(s["n_grad"])
    m = []
    for k in range(GAMMAS):
        acc = 0.0
        for b in range(BINS):
            acc += float(int(s["grad"][k][b])) * W[b]
        m.append(acc / float(n) if n else 0.0)
    return m


def best_gamma(p, m):
    best = 0
    for k in range(1, GAMMAS):
        if m[k] > m[best]:
            best = k
    if all(v == m[0] for v in m):
        return 1.0
    g = p.gamma[best]
    if 0 < best < GAMMAS - 1:
        x0, x1, x2 = math.log(p.gamma[best - 1]), math.log(p.gamma[best]), math.log(p.gamma[best + 1])
        d1, d2 = (m[best] - m[best - 1]) / (x1 - x0), (m[best + 1] - m[best]) / (x2 - x1)
        dd = (d2 - d1) / (x2 - x0)
        if dd != 0.0:
            g = math.exp(0.5 * (x0 + x1) - d1 / (2.0 * dd))
            g = min(max(g, p.gamma[best - 1]), p.gamma[best + 1])
    return g


def recommend(p, s, exposure):
    """(next exposure, gamma_hat)."""
    g = best_gamma(p, metric(p, s))
    return min(max(exposure * math.pow(g, -p.kp), p.e_min), p.e_max), g


def photograph(radiance, exposure):
    """The camera of the closed-loop tests: clip(255 radiance E), rounded down, as uint8."""
    return np.clip(255.0 * np.asarray(radiance, np.float64) * exposure, 0, 255).astype(np.uint8)
