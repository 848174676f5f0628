"""Independent reference of the intrinsic calibration and the generator of the synthetic cases its tests share.

The forward model restated in numpy with Rodrigues poses (the library keeps rotation matrices and the Cayley map), numeric
Jacobians by scipy, scipy's own optimisers: no code shared with chalkydri_amd.  solve() starts where ck_calib_init starts."""
import json
import os

import numpy as np
from scipy.optimize import least_squares

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calib_cameras.json")
NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")


def cameras():
    """The reference's three calib blobs (chalkydri.ron): name -> (k[9], width, height)."""
    out = {}
    for name, blob in json.load(open(GOLDEN)).items():
        m = blob["OpenCVModel5"]
        out[name] = (np.array([m[n] for n in NAMES], np.float64), int(m["width"]), int(m["height"]))
    return out


def board_points(rows=6, cols=6, tag_size=0.088, tag_spacing=0.3):
    """The 4 rows cols corners of an aprilgrid board, x right and y down in the board plane, tag (r, c) at c, r times the pitch;
    per tag in ck_detection_t's corner order (-1, 1), (1, 1), (1, -1), (-1, -1) times half the tag size about the tag's centre."""
    s, pitch = tag_size / 2, tag_size * (1 + tag_spacing)
    pts = []
    for r in range(rows):
        for c in range(cols):
            for dx, dy in ((-1, 1), (1, 1), (1, -1), (-1, -1)):
                pts.append((c * pitch + s + dx * s, r * pitch + s + dy * s))
    return np.array(pts, np.float64)


def rodrigues(rv):
    th = np.linalg.norm(rv)
    if th < 1e-300:
        return np.eye(3)
    n = rv / th
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def rotvec(R):
    """Inverse of rodrigues for angles below pi (the cases here are below 0.7 rad of tilt and any in-plane turn)."""
    c = np.clip((np.trace(R) - 1) / 2, -1, 1)
    th = np.arccos(c)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-12:
        return w / 2
    if np.pi - th < 1e-6:   # near a half turn: the axis from R + I
        M = (R + np.eye(3)) / 2
        n = np.sqrt(np.maximum(np.diag(M), 0))
        i = int(np.argmax(n))
        n = M[i] / n[i]
        return n / np.linalg.norm(n) * th
    return w / (2 * np.sin(th)) * th


def project(k, R, t, XY):
    P = XY @ R[:, :2].T + t
    x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    r2 = x * x + y * y
    rad = 1 + r2 * (k[4] + r2 * (k[5] + r2 * k[8]))
    xd = x * rad + 2 * k[6] * x * y + k[7] * (r2 + 2 * x * x)
    yd = y * rad + k[6] * (r2 + 2 * y * y) + 2 * k[7] * x * y
    return np.stack([k[0] * xd + k[2], k[1] * yd + k[3]], 1)


def make_case(k, w, h, n_frames, noise, seed, board=None, min_points=24):
    """Frames of the board under random poses: tilt up to 0.6 rad about a random in-plane axis, any in-plane turn, 0.45-0.9 m range,
    the board's centre seen in the middle half of the image; points within 4 px of the frame edge are dropped.  Returns a list of
    (board_xy [n][2], image_uv [n][2]) and the true poses (R, t)."""
    rng = np.random.default_rng([seed, n_frames, int(round(noise * 1000)), w])
    XY = board_points() if board is None else board
    ctr = XY.mean(0)
    frames, poses = [], []
    while len(frames) < n_frames:
        a, tilt, spin = rng.uniform(0, 2 * np.pi), rng.uniform(0, 0.6), rng.uniform(0, 2 * np.pi)
        R = rodrigues(tilt * np.array([np.cos(a), np.sin(a), 0.0])) @ rodrigues(np.array([0, 0, spin]))
        d = rng.uniform(0.45, 0.9)
        px = np.array([rng.uniform(0.25 * w, 0.75 * w), rng.uniform(0.25 * h, 0.75 * h)])
        ray = np.array([(px[0] - k[2]) / k[0], (px[1] - k[3]) / k[1], 1.0])
        t = d * ray / np.linalg.norm(ray) - R[:, :2] @ ctr
        uv = project(k, R, t, XY)
        keep = (uv[:, 0] >= 4) & (uv[:, 0] <= w - 1 - 4) & (uv[:, 1] >= 4) & (uv[:, 1] <= h - 1 - 4)
        # the polynomial model folds back far off the axis: keep what lies where the radial factor is still monotone in view
        P = XY @ R[:, :2].T + t
        keep &= P[:, 2] > 0.1
        if keep.sum() < min_points:
            continue
        uvn = uv[keep] + (rng.normal(0, noise, (int(keep.sum()), 2)) if noise > 0 else 0.0)
        frames.append((XY[keep].copy(), uvn))
        poses.append((R, t))
    return frames, poses


def pack(frames):
    """(board_xy, image_uv, frame_start) of a list of frames: the shared arrays of the C ABI."""
    starts = np.zeros(len(frames) + 1, np.int32)
    starts[1:] = np.cumsum([len(f[0]) for f in frames])
    return (np.ascontiguousarray(np.concatenate([f[0] for f in frames]), np.float64),
            np.ascontiguousarray(np.concatenate([f[1] for f in frames]), np.float64), starts)


def _unpack(x, n_frames, k0, free):
    k = k0.copy()
    k[free] = x[:len(free)]
    rest = x[len(free):].reshape(n_frames, 6)
    return k, rest


def residuals(x, frames, k0, free):
    k, rest = _unpack(x, len(frames), k0, free)
    out = []
    for (XY, uv), p in zip(frames, rest):
        out.append((project(k, rodrigues(p[:3]), p[3:], XY) - uv).ravel())
    return np.concatenate(out)


def solve(frames, cam0, poses0, fixed_mask=0, method="trf", max_nfev=None):
    """scipy's least_squares from the library's start (cam0 [9], poses0 [F][12]) -> (k [9], rms, scipy's result)."""
    free = [i for i in range(9) if not (fixed_mask >> i) & 1]
    k0 = np.asarray(cam0, np.float64).copy()
    x0 = [k0[free]]
    for P in np.asarray(poses0, np.float64).reshape(-1, 12):
        x0.append(rotvec(P[:9].reshape(3, 3)))
        x0.append(P[9:])
    x0 = np.concatenate(x0)
    kw = dict(x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, args=(frames, k0, free))
    if method == "trf":
        r = least_squares(residuals, x0, method="trf", max_nfev=max_nfev or 2000, **kw)
    else:
        r = least_squares(residuals, x0, method="lm", max_nfev=max_nfev or 200000, **kw)
    k, _ = _unpack(r.x, len(frames), k0, free)
    n = sum(len(f[0]) for f in frames)
    return k, float(np.sqrt(np.sum(r.fun ** 2) / n)), r
