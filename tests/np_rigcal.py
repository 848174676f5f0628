"""Independent reference of the mount calibration, written from the formulas and not from the C: numpy, Rodrigues
rotations, scipy.optimize.least_squares over numeric Jacobians (central differences, grouped by the sparsity of the problem: a
point touches one step and one camera).  Both costs: `angular` (point-to-ray distance over the range, the library's) and `object`
(point-to-ray distance in metres, the rig solver's).  Also the scene generator the CPU and GPU tests share.

Frames: world -> robot (R_s, t_s), p_robot = R_s X + t_s; camera c sits at o_c in the robot frame, p_cam = A_c (p_robot - o_c);
robot_to_cam = (A_c, b_c = -A_c o_c).  Robot x forward, y left, z up; camera x right, y down, z forward.
"""
import numpy as np
from scipy.optimize import least_squares

from np_rig import CORNERS, mat_to_quat, quat_to_mat, rot_z, small_rotation  # noqa: F401

A0 = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])      # camera axes of a camera that looks along robot x


def rodrigues(w):
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if a < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(a) / a) * K + ((1 - np.cos(a)) / (a * a)) * (K @ K)


def rodrigues_many(w):
    """[n][3] -> [n][3][3]"""
    return np.stack([rodrigues(v) for v in w]) if len(w) else np.zeros((0, 3, 3))


def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def room_tags(width=8.0, depth=6.0, spacing=1.0):
    """Tags on the four walls of a room, their normal (local x) into the room, heights alternating 0.6 / 1.2 m: [(R, t)]."""
    tags, k = [], 0
    walls = [((0, 0), (1, 0), np.pi / 2), ((width, 0), (0, 1), np.pi), ((width, depth), (-1, 0), -np.pi / 2), ((0, depth), (0, -1), 0.0)]
    for (x0, y0), (dx, dy), yaw in walls:
        length = width if dx else depth
        for d in np.arange(spacing / 2, length, spacing):
            tags.append((rot_z(yaw), np.array([x0 + dx * d, y0 + dy * d, 0.6 if k % 2 else 1.2])))
            k += 1
    return tags


def make_mounts(rng, n_cams):
    """n_cams cameras at different yaws, pitched up a little, within 0.3 m of the robot's centre: [(A, o)]."""
    out = []
    for c in range(n_cams):
        yaw = 2 * np.pi * c / n_cams + rng.uniform(-0.2, 0.2)
        body = rot_z(yaw) @ rot_y(-rng.uniform(0.05, 0.25)) @ small_rotation(rng, 0.05)       # robot <- camera body
        out.append((A0 @ body.T, np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.2, 0.6)])))
    return out


def perturb_mounts(rng, mounts, angle=np.radians(5.0), shift=0.05, keep=(0,)):
    """Start mounts off by up to `angle` and `shift` per axis; the cameras in `keep` stay."""
    out = []
    for c, (A, o) in enumerate(mounts):
        out.append((A, o) if c in keep else (A @ rodrigues(rng.uniform(-angle, angle, 3) / np.sqrt(3)), o + rng.uniform(-shift, shift, 3)))
    return out


def make_capture(rng, mounts, n_steps, tags=None, noise=0.0, half_fov=(0.7, 0.5), width=8.0, depth=6.0):
    """Robot poses on the floor of the room; a tag is seen when all four corners fall inside the pinhole's field of view
    (|x / z| < half_fov[0], |y / z| < half_fov[1]) from its front.  Returns (steps, truth): steps[s][c] = ([(R, t)], bearings
    (4 k, 3)), truth = [(R_s, t_s)] world -> robot, and the heading of every step."""
    tags = room_tags(width, depth) if tags is None else tags
    steps, truth, gyro = [], [], []
    for _ in range(n_steps):
        yaw = rng.uniform(-np.pi, np.pi)
        Rwr, pos = rot_z(yaw), np.array([rng.uniform(1.5, width - 1.5), rng.uniform(1.5, depth - 1.5), 0.0])
        R, t = Rwr.T, -Rwr.T @ pos
        cams = []
        for A, o in mounts:
            seen, bear = [], []
            for Rt, tt in tags:
                P = (((Rt @ CORNERS.T).T + tt) @ R.T + t - o) @ A.T
                cam_pos = Rwr @ o + pos
                if np.any(P[:, 2] < 0.3) or (Rt[:, 0] @ (cam_pos - tt)) / np.linalg.norm(cam_pos - tt) < 0.3:
                    continue
                xy = P[:, :2] / P[:, 2:3]
                if np.any(np.abs(xy[:, 0]) > half_fov[0]) or np.any(np.abs(xy[:, 1]) > half_fov[1]):
                    continue
                if noise > 0:
                    xy = xy + rng.normal(0, noise, xy.shape)
                v = np.concatenate([xy, np.ones((4, 1))], 1)
                seen.append((Rt, tt))
                bear.append(v / np.linalg.norm(v, axis=1, keepdims=True))
            cams.append((seen, np.concatenate(bear) if bear else np.zeros((0, 3))))
        steps.append(cams)
        truth.append((R, t))
        gyro.append(yaw)
    return steps, truth, np.array(gyro)


# ---- the problem ----------------------------------------------------------------------------------------------------------------
class Problem:
    """The points of the used steps (at least min_cams cameras with a tag) of `steps`, flat."""

    def __init__(self, steps, n_cams, min_cams=2):
        self.used = [s for s, cams in enumerate(steps) if sum(len(t) > 0 for t, _ in cams) >= min_cams]
        X, V, ci, si = [], [], [], []
        for u, s in enumerate(self.used):
            for c, (tg, bear) in enumerate(steps[s]):
                for k, (Rt, tt) in enumerate(tg):
                    X.append((Rt @ CORNERS.T).T + tt)
                    V.append(np.asarray(bear, float).reshape(-1, 3)[4 * k:4 * k + 4])
                    ci += [c] * 4
                    si += [u] * 4
        self.X, self.V = np.concatenate(X), np.concatenate(V)
        self.ci, self.si, self.n_cams = np.array(ci), np.array(si), n_cams

    def residuals(self, A, o, R, t, cost="angular"):
        """A [C][3][3], o [C][3], R [U][3][3], t [U][3] -> [P][3]"""
        q = np.einsum("pij,pj->pi", R[self.si], self.X) + t[self.si] - o[self.ci]
        p = np.einsum("pij,pj->pi", A[self.ci], q)
        v = self.V
        e = p - v * (np.sum(v * p, 1) / np.sum(v * v, 1))[:, None]
        return e / np.linalg.norm(p, axis=1)[:, None] if cost == "angular" else e

    def rms(self, A, o, R, t, cost="angular"):
        return float(np.sqrt(np.sum(self.residuals(A, o, R, t, cost) ** 2) / len(self.X)))


def solve(prob, mounts0, poses0, free, cost="angular", method="trf", tol=1e-15, max_nfev=400):
    """scipy's minimum from the start.  mounts0 [(A, o)], poses0 [(R, t)] of the USED steps, free [C][6] booleans (rotation about
    robot x y z, o x y z).  Returns (mounts [(A, o)], poses [(R, t)], rms, scipy's result)."""
    C, U = prob.n_cams, len(prob.used)
    A_0, o_0 = np.stack([m[0] for m in mounts0]), np.stack([m[1] for m in mounts0])
    R_0, t_0 = np.stack([p[0] for p in poses0]), np.stack([p[1] for p in poses0])
    free = np.asarray(free, bool).reshape(C, 6)
    fidx = np.flatnonzero(free.reshape(-1))

    def unpack(x):
        cam = np.zeros(6 * C)
        cam[fidx] = x[:len(fidx)]
        cam, st = cam.reshape(C, 6), x[len(fidx):].reshape(U, 6)
        A = np.einsum("cij,cjk->cik", A_0, rodrigues_many(cam[:, :3]))
        R = np.einsum("sij,sjk->sik", R_0, rodrigues_many(st[:, :3]))
        return A, o_0 + cam[:, 3:], R, t_0 + st[:, 3:]

    def fun(x):
        return prob.residuals(*unpack(x), cost).reshape(-1)

    def jac(x, h=1e-6):
        """central differences; the six parameters of all steps are perturbed together: a residual depends on one step only"""
        J = np.zeros((3 * len(prob.X), len(x)))
        for j in range(len(fidx)):
            d = np.zeros(len(x))
            d[j] = h
            J[:, j] = (fun(x + d) - fun(x - d)) / (2 * h)
        rows = np.arange(3 * len(prob.X))
        for k in range(6):
            d = np.zeros(len(x))
            d[len(fidx) + k::6] = h
            col = (fun(x + d) - fun(x - d)) / (2 * h)
            J[rows, len(fidx) + 6 * np.repeat(prob.si, 3) + k] = col
        return J

    x0 = np.zeros(len(fidx) + 6 * U)
    sol = least_squares(fun, x0, jac=jac, method=method, ftol=tol, xtol=tol, gtol=tol, max_nfev=max_nfev)
    A, o, R, t = unpack(sol.x)
    return list(zip(A, o)), list(zip(R, t)), prob.rms(A, o, R, t, cost), sol


def mount_distance(m1, m2):
    """(angle between the rotations in radians, distance of the positions in metres); the angle from the skew part of the relative
    rotation, which resolves angles far below the 1e-8 at which arccos of the trace stops"""
    Rd = m1[0].T @ m2[0]
    w = 0.5 * np.array([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]])
    return float(np.arctan2(np.linalg.norm(w), (np.trace(Rd) - 1) / 2)), float(np.linalg.norm(m1[1] - m2[1]))


def numeric_jacobian(mount, pose, X, v, h):
    """Central differences of the angular residual of one view's points with respect to the library's increments (camera: A C(dw),
    o + do; step: R C(dw), t + dt; to first order C(dw) = Rodrigues(dw)): [n][3][12]."""
    A, o = mount
    R, t = pose
    X, v = np.asarray(X, float).reshape(-1, 3), np.asarray(v, float).reshape(-1, 3)

    def res(d):
        Ad, od, Rd, td = A @ rodrigues(d[0:3]), o + d[3:6], R @ rodrigues(d[6:9]), t + d[9:12]
        p = ((X @ Rd.T + td) - od) @ Ad.T
        e = p - v * (np.sum(v * p, 1) / np.sum(v * v, 1))[:, None]
        return e / np.linalg.norm(p, axis=1)[:, None]

    J = np.zeros((len(X), 3, 12))
    for k in range(12):
        d = np.zeros(12)
        d[k] = h
        J[:, :, k] = (res(d) - res(-d)) / (2 * h)
    return J


def synthetic_capture(rng, n_cams, n_steps, n_tags, noise=1e-3):
    """A capture of chosen shape for the tests of the device mapping: any mounts, any robot poses, n_tags(s, c) tags 1..5 m in front
    of camera c at step s (0: the camera sees nothing there).  Returns (steps as make_capture, mounts [(A, o)], poses [(R, t)])."""
    from np_rig import CV_FROM_TAG, random_rotation
    mounts = [(random_rotation(rng), rng.uniform(-0.4, 0.4, 3)) for _ in range(n_cams)]
    steps, poses = [], []
    for s in range(n_steps):
        Rwr, pos = rot_z(rng.uniform(-np.pi, np.pi)) @ small_rotation(rng, 0.1), np.array([rng.uniform(2, 14), rng.uniform(1, 7), rng.uniform(-0.1, 0.1)])
        R, t = Rwr.T, -Rwr.T @ pos
        cams = []
        for c, (A, o) in enumerate(mounts):
            tags, bear = [], []
            for _ in range(int(n_tags(s, c))):
                z = rng.uniform(1.0, 5.0)
                pc = np.array([rng.uniform(-0.4, 0.4) * z, rng.uniform(-0.3, 0.3) * z, z])
                Rtc = small_rotation(rng, 0.5) @ CV_FROM_TAG               # cam <- tag
                Rcw, tcw = A @ R, A @ (t - o)                              # cam <- world
                Rtw, ttw = Rcw.T @ Rtc, Rcw.T @ (pc - tcw)
                P = ((Rtw @ CORNERS.T).T + ttw) @ Rcw.T + tcw
                xy = P[:, :2] / P[:, 2:3] + rng.normal(0, noise, (4, 2))
                v = np.concatenate([xy, np.ones((4, 1))], 1)
                tags.append((Rtw, ttw))
                bear.append(v / np.linalg.norm(v, axis=1, keepdims=True))
            cams.append((tags, np.concatenate(bear) if bear else np.zeros((0, 3))))
        steps.append(cams)
        poses.append((R, t))
    return steps, mounts, poses


def perturb_poses(rng, poses, angle=0.02, shift=0.03):
    return [(R @ rodrigues(rng.uniform(-angle, angle, 3)), t + rng.uniform(-shift, shift, 3)) for R, t in poses]
