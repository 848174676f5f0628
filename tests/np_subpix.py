"""The sub-pixel corner refinement of DESIGN.md §4q restated in numpy (test infrastructure, CPU only), independently of
csrc/ck_subpix_math.h: the window is built as arrays and the sums are numpy's, so the summation order is NOT the library's — the
results agree to rounding, not to the bit.

Coordinates: pixel (i, j) covers [i, i + 1) x [j, j + 1), so the image is sampled at (x - 0.5, y - 0.5) in pixel-index space,
bilinearly, indices clamped to the frame.  One iteration at the estimate q: the bilinear patch of (2w + 3)^2 samples at q + integer
offsets, central differences g = (P[+1] - P[-1]) / 2 on the inner (2w + 1)^2 taps, weights m = exp(-(dx / w)^2) exp(-(dy / w)^2),
sums a = sum m gx^2, b = sum m gx gy, c = sum m gy^2, b1 = sum m (gx^2 px + gx gy py), b2 = sum m (gx gy px + gy^2 py) with p the
tap's offset, det = a c - b^2; |det| <= det_min: FLAT (the input comes back); step ((c b1 - b b2) / det, (a b2 - b b1) / det); stop
when |step|^2 <= eps^2 or after max_iters steps; a point that ended more than w from its start on either axis comes back as it
went in (REJECTED).
"""
import numpy as np

CONVERGED, MAXIT, FLAT, REJECTED = 0, 1, 2, 3


def weights(w):
    d = np.arange(-w, w + 1) / w
    e = np.exp(-d * d)
    return np.outer(e, e)


def _axis(v, size, n):
    """indices and fraction of n + 1 consecutive pixel columns from floor(v) (v kept within 32 pixels of the frame, as the library does)"""
    v = min(max(v, -32.0), size + 32.0)
    i0 = int(np.floor(v))
    return np.clip(i0 + np.arange(n + 1), 0, size - 1), v - i0


def patch(img, x, y, w):
    """bilinear samples at (x + i, y + j), i, j = -(w + 1) .. w + 1: [2w + 3][2w + 3], rows = y"""
    n = 2 * w + 3
    h, wd = img.shape
    xi, fx = _axis(x - 0.5 - (w + 1), wd, n)
    yi, fy = _axis(y - 0.5 - (w + 1), h, n)
    # (the clamp of v is applied to the patch's first sample here and to the estimate in the library: the same thing inside the range
    # the tests use, where neither acts)
    p = img[np.ix_(yi, xi)].astype(np.float64)
    top = p[:-1, :-1] * (1 - fx) + p[:-1, 1:] * fx
    bot = p[1:, :-1] * (1 - fx) + p[1:, 1:] * fx
    return top * (1 - fy) + bot * fy


def refine(img, x0, y0, w=5, max_iters=30, eps=1e-3, det_min=1e-2):
    """(x, y, status, iters)"""
    m = weights(w)
    py, px = np.mgrid[-w:w + 1, -w:w + 1].astype(np.float64)
    x, y, status, it = float(x0), float(y0), MAXIT, 0
    while it < max_iters:
        P = patch(img, x, y, w)
        gx = (P[1:-1, 2:] - P[1:-1, :-2]) * 0.5
        gy = (P[2:, 1:-1] - P[:-2, 1:-1]) * 0.5
        a, b, c = (m * gx * gx).sum(), (m * gx * gy).sum(), (m * gy * gy).sum()
        b1 = (m * (gx * gx * px + gx * gy * py)).sum()
        b2 = (m * (gx * gy * px + gy * gy * py)).sum()
        det = a * c - b * b
        if abs(det) <= det_min:
            status = FLAT
            break
        dx, dy = (c * b1 - b * b2) / det, (a * b2 - b * b1) / det
        x, y, it = x + dx, y + dy, it + 1
        if dx * dx + dy * dy <= eps * eps:
            status = CONVERGED
            break
    if status != FLAT and not (abs(x - x0) <= w and abs(y - y0) <= w):
        status = REJECTED
    if status in (FLAT, REJECTED):
        return float(x0), float(y0), status, it
    return x, y, status, it


def refine_many(img, xy, **kw):
    out = np.array([refine(img, x, y, **kw) for x, y in np.asarray(xy, float).reshape(-1, 2)])
    return out[:, :2], out[:, 2].astype(int), out[:, 3].astype(int)
