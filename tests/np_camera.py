"""An independent numpy restatement of the EUCM / UCM camera model (Khomutenko, Garcia & Martinet 2016), written from the formulas of
DESIGN.md §4p and from nothing in chalkydri_amd/csrc: the specification the host functions are tested against.

A lens is (fx, fy, cx, cy, alpha, beta); UCM is beta = 1.
"""
import numpy as np

# the lenses of the tests: the wide EUCM of DESIGN.md §4p (image corner of 1280 x 800 about 87 degrees off axis), a UCM, a mild one
LENSES = {"eucm_wide": (500.0, 502.0, 640.0, 400.0, 0.62, 1.08),
          "ucm": (700.0, 700.0, 630.0, 410.0, 0.55, 1.0),
          "eucm_mild": (600.0, 598.0, 645.0, 395.0, 0.3, 1.15)}
W, H = 1280, 800


def grid(step=16, w=W, h=H):
    ys, xs = np.mgrid[0:h + 1:step, 0:w + 1:step]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)


def ray(lens, px):
    """(mx, my, kz, inside): a point on each pixel's ray and whether the pixel lies inside the model's valid disc."""
    fx, fy, cx, cy, alpha, beta = lens
    px = np.asarray(px, np.float64).reshape(-1, 2)
    mx, my = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
    r2 = mx * mx + my * my
    inside = np.ones(len(px), bool)
    if alpha > 0.5:
        inside = r2 < 1.0 / (beta * (2.0 * alpha - 1.0))
    with np.errstate(all="ignore"):
        s = np.sqrt(1.0 - (2.0 * alpha - 1.0) * beta * r2)
        kz = (1.0 - alpha * alpha * beta * r2) / (alpha * s + (1.0 - alpha))
    return mx, my, kz, inside


def unproject(lens, px):
    """(unit bearings [n][3], ok [n]); the bearings of pixels that are not ok are zero."""
    mx, my, kz, inside = ray(lens, px)
    with np.errstate(all="ignore"):
        v = np.stack([mx, my, kz], 1)
        b = v / np.linalg.norm(v, axis=1)[:, None]
    ok = inside & np.all(np.isfinite(b), 1)
    b[~inside] = 0.0
    return b, ok


def normalize(lens, px):
    """(normalised points [n][2], ok [n]): the ray must also point forward (kz > 0)."""
    mx, my, kz, inside = ray(lens, px)
    ok = inside & (kz > 0)
    with np.errstate(all="ignore"):
        xy = np.stack([mx / kz, my / kz], 1)
    ok &= np.all(np.isfinite(xy), 1)
    xy[~ok] = 0.0
    return xy, ok


def project(lens, xyz):
    """(pixels [n][2], ok [n]); pixels of points that do not project are zero."""
    fx, fy, cx, cy, alpha, beta = lens
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        d = np.sqrt(beta * (X * X + Y * Y) + Z * Z)
        den = alpha * d + (1.0 - alpha) * Z
        w = (1.0 - alpha) / alpha if alpha > 0.5 else alpha / (1.0 - alpha)
        ok = (den > 0) & (Z > -w * d)
        uv = np.stack([fx * X / den + cx, fy * Y / den + cy], 1)
    ok &= np.all(np.isfinite(uv), 1)
    uv[~ok] = 0.0
    return uv, ok


def off_axis_deg(lens, px):
    b, _ = unproject(lens, px)
    return np.degrees(np.arccos(np.clip(b[:, 2], -1, 1)))
