"""The rig pose refinement restated in numpy, independent of the C text: the angular residual, both parametrisations,
the heading prior, the minimum by scipy.optimize.least_squares, and the Jacobian by central differences in the world-axes tangent of the
world <- robot pose (R <- Exp(dw) R, p <- p + dp; ordered x, y, z, wx, wy, wz).  Also the scenes the tests share.

A scene is `cams` as tests/np_rig.py takes them: per camera (tags [(R, t)], bearings (4 n, 3), (A, b)) with p_cam = A p_robot + b."""
import numpy as np
from scipy.optimize import least_squares

import np_rig as N

FREE, PLANAR = 0, 1


def exp_so3(w):
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if a < 1e-12:
        return np.eye(3) + K + K @ K / 2
    return np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / (a * a) * K @ K


def points(cams, rejected=None):
    """(X world corners, v bearings, A, o of every used point's camera, camera numbers); rejected[c] = set of deleted tags"""
    X, V, As, Os, Cs = [], [], [], [], []
    for c, (tags, b, (A, bb)) in enumerate(cams):
        b = np.asarray(b, float).reshape(-1, 3)
        o = -A.T @ bb
        for t, (R, tt) in enumerate(tags):
            if rejected is not None and t in rejected[c]:
                continue
            for j in range(4):
                X.append(R @ N.CORNERS[j] + tt)
                V.append(b[4 * t + j])
                As.append(A)
                Os.append(o)
                Cs.append(c)
    return np.array(X).reshape(-1, 3), np.array(V).reshape(-1, 3), np.array(As).reshape(-1, 3, 3), np.array(Os).reshape(-1, 3), np.array(Cs, int)


def bearing_residuals(pts, R_wr, p):
    """e = (p_cam - v (v.p_cam) / (v.v)) / |p_cam| of every point, (N, 3); and v.p_cam"""
    X, V, A, O, _ = pts
    q = (X - p) @ R_wr - O                       # R_wr^T (X - p) - o
    pc = np.einsum("nij,nj->ni", A, q)
    vp = np.einsum("ni,ni->n", V, pc)
    f = vp / np.einsum("ni,ni->n", V, V)
    return (pc - V * f[:, None]) / np.linalg.norm(pc, axis=1)[:, None], vp


def prior_residual(R_wr, gyro, gyro_sigma):
    return (R_wr[1, 0] * np.cos(gyro) - R_wr[0, 0] * np.sin(gyro)) / gyro_sigma


def project_planar(R_wr, p, z):
    """the planar start of a pose: (x, y, theta), z given"""
    return np.array([p[0], p[1], np.arctan2(R_wr[1, 0], R_wr[0, 0])])


def pose_of(mode, x, base, z):
    """world <- robot of the unknowns x: free (dw, dp) about base = (R, p); planar (x, y, theta)"""
    if mode == PLANAR:
        return N.rot_z(x[2]), np.array([x[0], x[1], z])
    return exp_so3(x[:3]) @ base[0], base[1] + x[3:]


def stacked(pts, R_wr, p, sigma, gyro, gyro_sigma):
    """the residual vector in units of radians: the bearing rows, then the prior's row times sigma / gyro_sigma"""
    e, _ = bearing_residuals(pts, R_wr, p)
    r = e.reshape(-1)
    if gyro_sigma > 0:
        r = np.append(r, sigma * prior_residual(R_wr, gyro, gyro_sigma))
    return r


def minimise(cams, R0, p0, mode=FREE, sigma=1e-3, gyro=0.0, gyro_sigma=0.0, z=0.0, rejected=None):
    """scipy's minimum from the start (R0, p0) (world <- robot).  Returns (R_wr, p, cost of the bearing rows)."""
    pts = points(cams, rejected)
    base = (np.asarray(R0, float), np.asarray(p0, float))
    x = project_planar(base[0], base[1], z) if mode == PLANAR else np.zeros(6)

    def fun(x):
        R, p = pose_of(mode, x, base, z)
        return stacked(pts, R, p, sigma, gyro, gyro_sigma) / sigma
    for _ in range(3):                           # restarts re-centre the free parametrisation and tighten the stop
        sol = least_squares(fun, x, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale="jac", max_nfev=2000)
        R, p = pose_of(mode, sol.x, base, z)
        if mode == FREE:
            base, x = (R, p), np.zeros(6)
        else:
            x = sol.x
    for _ in range(4):                           # Gauss-Newton steps on central differences: MINPACK stops a little short of 1e-9
        J = np.array([(fun(x + d) - fun(x - d)) / 2e-6 for d in 1e-6 * np.eye(len(x))]).T
        x = x - np.linalg.lstsq(J, fun(x), rcond=None)[0]
        R, p = pose_of(mode, x, base, z)
        if mode == FREE:
            base, x = (R, p), np.zeros(6)
    e, _ = bearing_residuals(pts, R, p)
    return R, p, float((e * e).sum())


def tangent_jacobian(cams, R_wr, p, sigma=1e-3, gyro=0.0, gyro_sigma=0.0, rejected=None, h=1e-6):
    """d stacked / d (x, y, z, wx, wy, wz) by central differences at (R_wr, p)"""
    pts = points(cams, rejected)
    cols = []
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        rp = stacked(pts, exp_so3(d[3:]) @ R_wr, p + d[:3], sigma, gyro, gyro_sigma)
        rm = stacked(pts, exp_so3(-d[3:]) @ R_wr, p - d[:3], sigma, gyro, gyro_sigma)
        cols.append((rp - rm) / (2 * h))
    return np.array(cols).T


def covariance(cams, R_wr, p, mode=FREE, sigma=1e-3, gyro=0.0, gyro_sigma=0.0, rejected=None):
    """sigma^2 (J^T J)^-1 as a 6 x 6 in the tangent's order; planar: over x, y, wz, zero elsewhere"""
    J = tangent_jacobian(cams, R_wr, p, sigma, gyro, gyro_sigma, rejected)
    keep = [0, 1, 5] if mode == PLANAR else list(range(6))
    C = np.zeros((6, 6))
    C[np.ix_(keep, keep)] = sigma * sigma * np.linalg.inv(J[:, keep].T @ J[:, keep])
    return C


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
FRONT = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])   # camera x right, y down, z forward; looks along robot +x
LEFT = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])     # looks along robot +y
FACING_MINUS_X = N.rot_z(np.pi)                                            # a tag's normal is its local x
FACING_MINUS_Y = N.rot_z(-np.pi / 2)
TRUTH = (2.0, 0.3, 0.1)                                                    # the robot of every scene: x, y, yaw; it stands on z = 0
NOISE = 5e-4


def mount(A, o):
    A = np.asarray(A, float)
    return A, -A @ np.asarray(o, float)


SCENES = {
    "near_far": [(mount(FRONT, (0, 0, 0.5)), [(FACING_MINUS_X, (3.5, 0.5, 0.8)), (FACING_MINUS_X, (8.0, -1.0, 1.2))])],
    "wall": [(mount(FRONT, (0, 0, 0.5)), [(FACING_MINUS_X, (5.0, -1.0, 0.6)), (FACING_MINUS_X, (5.0, 0.3, 1.0)), (FACING_MINUS_X, (5.0, 1.5, 0.8))])],
    "far_single": [(mount(FRONT, (0, 0, 0.5)), [(FACING_MINUS_X, (8.0, 0.3, 1.0))])],
    "two_cameras": [(mount(FRONT, (0.2, 0.0, 0.5)), [(FACING_MINUS_X, (4.5, 0.8, 0.9))]),
                    (mount(LEFT, (0.0, 0.2, 0.4)), [(FACING_MINUS_Y, (2.5, 3.5, 1.0)), (FACING_MINUS_Y, (1.2, 4.5, 0.7))])],
    "single_3m": [(mount(FRONT, (0, 0, 0.5)), [(FACING_MINUS_X, (5.0, 0.3, 1.0))])],
}


def truth_pose(truth=TRUTH):
    return N.rot_z(truth[2]), np.array([truth[0], truth[1], 0.0])


def render(scene, rng=None, noise=0.0, truth=TRUTH):
    """cams of a scene seen from the true pose, the unit bearings plus `noise` per component"""
    R_wr, p = truth_pose(truth)
    cams = []
    for (A, b), tags in scene:
        tags = [(np.asarray(R, float), np.asarray(t, float)) for R, t in tags]
        bear = []
        for R, t in tags:
            for j in range(4):
                pc = A @ (R_wr.T @ (R @ N.CORNERS[j] + t - p)) + b
                v = pc / np.linalg.norm(pc)
                bear.append(v + (rng.normal(0.0, noise, 3) if noise > 0 else 0.0))
        cams.append((tags, np.array(bear).reshape(-1, 3), (A, b)))
    return cams


TAG_IN_CAMERA = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0]])   # a tag's normal (local x) looks down the camera's -z


def instant(counts, rng, n_cams=None, noise=NOISE):
    """cams of one instant of the robot at TRUTH: camera c (0.5 m up, looking along the robot's x turned by -45 degrees times c) sees
    counts[c] tags 3 .. 6 m away that face it; padded with empty cameras to n_cams"""
    R_wr, p = truth_pose()
    counts = list(counts) + [0] * ((n_cams or len(counts)) - len(counts))
    scene = []
    for c, k in enumerate(counts):
        Am, b = mount(FRONT @ N.rot_z(-np.pi / 4 * c), (0.1 * c, 0.05 * c, 0.5))
        o = -Am.T @ b
        tags = []
        for t in range(k):
            pc = np.array([-1.5 + 0.4 * (t % 8), -0.6 + 0.25 * ((t // 8) % 8), 3.0 + 0.37 * (t % 9)])
            tags.append((R_wr @ Am.T @ TAG_IN_CAMERA, R_wr @ (Am.T @ pc + o) + p))
        scene.append(((Am, b), tags))
    return render(scene, rng, noise)
