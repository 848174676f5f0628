"""The reference of the EUCM / UCM calibration tests: captures synthesised with the numpy restatement of the model (tests/np_camera.py)
and scipy's least_squares over (fx fy cx cy alpha [beta], Rodrigues poses) with numeric Jacobians: no code shared with the library."""
import numpy as np
from scipy.optimize import least_squares

import np_calib as N
import np_camera as NC


def project(lens, R, t, XY):
    P = XY @ R[:, :2].T + t
    return NC.project(lens, P)


def make_case(lens, n_frames, noise, seed, w=NC.W, h=NC.H, min_points=24, board=None, tilt_max=0.6, spread=0.25):
    """Frames of the board (np_calib.board_points) under random poses, as np_calib.make_case makes them for the polynomial model: tilt
    up to tilt_max about a random in-plane axis, any in-plane turn, 0.25-0.6 m range (a wide lens fills its image only from close by),
    the board's centre seen in the middle half of the image (spread 0.25: within that fraction of the size from the centre); points within 4 px of the frame edge, or that do not project, are dropped.
    Returns a list of (board_xy [n][2], image_uv [n][2]) and the true poses (R, t)."""
    rng = np.random.default_rng([seed, n_frames, int(round(noise * 1000)), int(lens[0])])
    XY = N.board_points() if board is None else board
    ctr = XY.mean(0)
    frames, poses = [], []
    while len(frames) < n_frames:
        a, tilt, spin = rng.uniform(0, 2 * np.pi), rng.uniform(0, tilt_max), rng.uniform(0, 2 * np.pi)
        R = N.rodrigues(tilt * np.array([np.cos(a), np.sin(a), 0.0])) @ N.rodrigues(np.array([0, 0, spin]))
        d = rng.uniform(0.25, 0.6)
        px = np.array([[rng.uniform((0.5 - spread) * w, (0.5 + spread) * w), rng.uniform((0.5 - spread) * h, (0.5 + spread) * h)]])
        ray = NC.unproject(lens, px)[0][0]
        t = d * ray - R[:, :2] @ ctr
        uv, ok = project(lens, R, t, XY)
        keep = ok & (uv[:, 0] >= 4) & (uv[:, 0] <= w - 1 - 4) & (uv[:, 1] >= 4) & (uv[:, 1] <= h - 1 - 4)
        if keep.sum() < min_points:
            continue
        uvn = uv[keep] + (rng.normal(0, noise, (int(keep.sum()), 2)) if noise > 0 else 0.0)
        frames.append((XY[keep].copy(), uvn))
        poses.append((R, t))
    return frames, poses


def pose12(R, t):
    return np.concatenate([np.asarray(R).ravel(), np.asarray(t)])


def _residuals(x, frames, nk):
    lens = tuple(x[:nk]) + ((1.0,) if nk == 5 else ())
    out = []
    for (XY, uv), p in zip(frames, x[nk:].reshape(len(frames), 6)):
        out.append((project(lens, N.rodrigues(p[:3]), p[3:], XY)[0] - uv).ravel())
    return np.concatenate(out)


def solve(frames, k0, poses0, ucm=False):
    """scipy's least_squares (trf, numeric Jacobian) from a start (k0 [>= 6], poses0 [F][12]) -> (k [6], rms, scipy's result)."""
    nk = 5 if ucm else 6
    x0 = [np.asarray(k0, np.float64)[:nk]]
    for P in np.asarray(poses0, np.float64).reshape(-1, 12):
        x0.append(N.rotvec(P[:9].reshape(3, 3)))
        x0.append(P[9:])
    r = least_squares(_residuals, np.concatenate(x0), method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000,
                      args=(frames, nk))
    k = np.concatenate([r.x[:nk], [1.0] if ucm else []])
    n = sum(len(f[0]) for f in frames)
    return k, float(np.sqrt(np.sum(r.fun ** 2) / n)), r
