"""Independent reference of the field calibration, written from the formulas and not from the C: numpy, Rodrigues
rotations, scipy.optimize.least_squares over numeric Jacobians (central differences, grouped by the sparsity of the problem: a
point touches one step and one tag).  Also the scene generators the CPU and GPU tests share.  Does not import the library.

Frames as in np_rigcal.py: world -> robot (R_s, t_s), camera c at o_c in the robot frame, p_cam = A_c (R_s X + t_s - o_c).  A tag
is (Q, c): its corner x (np_rig.CORNERS, the tag's own frame) is at X = Q x + c.
"""
import numpy as np
from scipy.optimize import least_squares

from np_rig import CORNERS, mat_to_quat, quat_to_mat, random_rotation, rot_z, small_rotation  # noqa: F401
from np_rigcal import make_mounts, perturb_poses, rodrigues, rodrigues_many, room_tags  # noqa: F401


def perturb_layout(rng, layout, angle=np.radians(2.0), shift=0.03, keep=(0,)):
    """Every tag moved by up to `shift` per axis and turned by up to `angle` about its own axes; the tags in `keep` stay."""
    return [(Q, c) if k in keep else (Q @ rodrigues(rng.uniform(-angle, angle, 3) / np.sqrt(3)), c + rng.uniform(-shift, shift, 3))
            for k, (Q, c) in enumerate(layout)]


def make_capture(rng, mounts, layout, n_steps, noise=0.0, half_fov=(0.7, 0.5), width=8.0, depth=6.0):
    """np_rigcal.make_capture with the tags' numbers kept: robot poses on the floor of the room; a tag is seen when all four corners
    fall inside the pinhole's field of view from its front.  Returns (steps, truth, gyro): steps[s][c] = (tag numbers, bearings (4 k, 3))."""
    steps, truth, gyro = [], [], []
    for _ in range(n_steps):
        yaw = rng.uniform(-np.pi, np.pi)
        Rwr, pos = rot_z(yaw), np.array([rng.uniform(1.5, width - 1.5), rng.uniform(1.5, depth - 1.5), 0.0])
        R, t = Rwr.T, -Rwr.T @ pos
        cams = []
        for A, o in mounts:
            seen, bear = [], []
            for k, (Q, c) in enumerate(layout):
                P = (((Q @ CORNERS.T).T + c) @ R.T + t - o) @ A.T
                cam_pos = Rwr @ o + pos
                if np.any(P[:, 2] < 0.3) or (Q[:, 0] @ (cam_pos - c)) / np.linalg.norm(cam_pos - c) < 0.3:
                    continue
                xy = P[:, :2] / P[:, 2:3]
                if np.any(np.abs(xy[:, 0]) > half_fov[0]) or np.any(np.abs(xy[:, 1]) > half_fov[1]):
                    continue
                if noise > 0:
                    xy = xy + rng.normal(0, noise, xy.shape)
                v = np.concatenate([xy, np.ones((4, 1))], 1)
                seen.append(k)
                bear.append(v / np.linalg.norm(v, axis=1, keepdims=True))
            cams.append((seen, np.concatenate(bear) if bear else np.zeros((0, 3))))
        steps.append(cams)
        truth.append((R, t))
        gyro.append(yaw)
    return steps, truth, np.array(gyro)


def synthetic_capture(rng, n_cams, n_steps, n_layout, seen, noise=1e-3):
    """A capture of chosen shape for the tests of the device mapping: tags anywhere on a ring of 6 m, any mounts, robot poses within
    3 m of the centre; camera c at step s has the tags seen(s, c) (a list of layout entries) wherever they are: a bearing is any
    direction, off by `noise`.  Returns (steps, mounts [(A, o)], layout [(Q, c)], poses [(R, t)])."""
    mounts = [(random_rotation(rng), rng.uniform(-0.4, 0.4, 3)) for _ in range(n_cams)]
    layout = [(random_rotation(rng), np.array([6 * np.cos(2 * np.pi * k / n_layout), 6 * np.sin(2 * np.pi * k / n_layout), rng.uniform(0.3, 1.5)]))
              for k in range(n_layout)]
    steps, poses = [], []
    for s in range(n_steps):
        Rwr, pos = rot_z(rng.uniform(-np.pi, np.pi)) @ small_rotation(rng, 0.1), np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-0.1, 0.1)])
        R, t = Rwr.T, -Rwr.T @ pos
        cams = []
        for c, (A, o) in enumerate(mounts):
            ids, bear = [int(k) for k in seen(s, c)], []
            for k in ids:
                Q, cc = layout[k]
                P = (((Q @ CORNERS.T).T + cc) @ R.T + t - o) @ A.T
                v = P / np.linalg.norm(P, axis=1, keepdims=True) + rng.normal(0, noise, (4, 3))
                bear.append(v / np.linalg.norm(v, axis=1, keepdims=True))
            cams.append((ids, np.concatenate(bear) if bear else np.zeros((0, 3))))
        steps.append(cams)
        poses.append((R, t))
    return steps, mounts, layout, poses


# ---- the problem ----------------------------------------------------------------------------------------------------------------
class Problem:
    """The points of the used steps (at least min_tags distinct tags over all cameras) of `steps`, flat."""

    def __init__(self, steps, mounts, n_layout, min_tags=2):
        self.used = [s for s, cams in enumerate(steps) if len({k for ids, _ in cams for k in ids}) >= min_tags]
        x, V, ci, si, ki = [], [], [], [], []
        for u, s in enumerate(self.used):
            for c, (ids, bear) in enumerate(steps[s]):
                for j, k in enumerate(ids):
                    x.append(CORNERS)
                    V.append(np.asarray(bear, float).reshape(-1, 3)[4 * j:4 * j + 4])
                    ci += [c] * 4
                    si += [u] * 4
                    ki += [k] * 4
        self.x, self.V = np.concatenate(x), np.concatenate(V)
        self.ci, self.si, self.ki = np.array(ci), np.array(si), np.array(ki)
        self.A, self.o = np.stack([m[0] for m in mounts]), np.stack([m[1] for m in mounts])
        self.n_layout = n_layout
        self.sightings = np.bincount(self.ki, minlength=n_layout) // 4

    def residuals(self, Q, c, R, t):
        """Q [L][3][3], c [L][3], R [U][3][3], t [U][3] -> [P][3]"""
        X = np.einsum("pij,pj->pi", Q[self.ki], self.x) + c[self.ki]
        q = np.einsum("pij,pj->pi", R[self.si], X) + t[self.si] - self.o[self.ci]
        p = np.einsum("pij,pj->pi", self.A[self.ci], q)
        v = self.V
        e = p - v * (np.sum(v * p, 1) / np.sum(v * v, 1))[:, None]
        return e / np.linalg.norm(p, axis=1)[:, None]

    def rms(self, Q, c, R, t):
        return float(np.sqrt(np.sum(self.residuals(Q, c, R, t) ** 2) / len(self.x)))

    def tag_rms(self, Q, c, R, t):
        e2 = np.sum(self.residuals(Q, c, R, t) ** 2, 1)
        return np.array([np.sqrt(np.sum(e2[self.ki == k]) / max(np.sum(self.ki == k), 1)) for k in range(self.n_layout)])


def solve(prob, layout0, poses0, free, method="trf", tol=1e-15, max_nfev=400):
    """scipy's minimum from the start.  layout0 [(Q, c)], poses0 [(R, t)] of the USED steps, free [L][6] booleans (rotation about the
    tag's own x y z, c x y z; a tag without sightings must be all False).  Returns (layout [(Q, c)], poses [(R, t)], rms, scipy's
    result)."""
    L, U = prob.n_layout, len(prob.used)
    Q_0, c_0 = np.stack([m[0] for m in layout0]), np.stack([m[1] for m in layout0])
    R_0, t_0 = np.stack([p[0] for p in poses0]), np.stack([p[1] for p in poses0])
    free = np.asarray(free, bool).reshape(L, 6)
    fidx = np.flatnonzero(free.reshape(-1))
    nf = len(fidx)

    def unpack(x):
        tg = np.zeros(6 * L)
        tg[fidx] = x[:nf]
        tg, st = tg.reshape(L, 6), x[nf:].reshape(U, 6)
        Q = np.einsum("kij,kjl->kil", Q_0, rodrigues_many(tg[:, :3]))
        R = np.einsum("sij,sjk->sik", R_0, rodrigues_many(st[:, :3]))
        return Q, c_0 + tg[:, 3:], R, t_0 + st[:, 3:]

    def fun(x):
        return prob.residuals(*unpack(x)).reshape(-1)

    where = np.full(6 * L, -1)
    where[fidx] = np.arange(nf)

    def jac(x, h=1e-6):
        """central differences; parameter a of all tags is perturbed together, and of all steps: a residual depends on one of each"""
        J = np.zeros((3 * len(prob.x), len(x)))
        rows = np.arange(3 * len(prob.x))
        for a in range(6):
            cols = where[6 * np.repeat(prob.ki, 3) + a]
            d = np.zeros(len(x))
            d[where[a::6][where[a::6] >= 0]] = h
            col = (fun(x + d) - fun(x - d)) / (2 * h)
            J[rows[cols >= 0], cols[cols >= 0]] = col[cols >= 0]
            d = np.zeros(len(x))
            d[nf + a::6] = h
            col = (fun(x + d) - fun(x - d)) / (2 * h)
            J[rows, nf + 6 * np.repeat(prob.si, 3) + a] = col
        return J

    x0 = np.zeros(nf + 6 * U)
    sol = least_squares(fun, x0, jac=jac, method=method, ftol=tol, xtol=tol, gtol=tol, max_nfev=max_nfev)
    Q, c, R, t = unpack(sol.x)
    return list(zip(Q, c)), list(zip(R, t)), prob.rms(Q, c, R, t), sol


def tag_distance(a, b):
    """(angle between the rotations in radians, distance of the positions in metres), the angle from the skew part of the relative
    rotation"""
    Rd = a[0].T @ b[0]
    w = 0.5 * np.array([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]])
    return float(np.arctan2(np.linalg.norm(w), (np.trace(Rd) - 1) / 2)), float(np.linalg.norm(a[1] - b[1]))


def layout_distance(a, b, which=None):
    """the largest angle or distance over the tags (those in `which`)"""
    ks = range(len(a)) if which is None else which
    return max(max(tag_distance(a[k], b[k])) for k in ks)


def numeric_jacobian(mount, pose, tag, v, h):
    """Central differences of the angular residual of one sighting's four corners with respect to the library's increments (tag:
    Q C(dw), c + dc; step: R C(dw), t + dt; to first order C(dw) = Rodrigues(dw)): [4][3][12]."""
    A, o = mount
    R, t = pose
    Q, c = tag
    v = np.asarray(v, float).reshape(-1, 3)

    def res(d):
        Qd, cd, Rd, td = Q @ rodrigues(d[0:3]), c + d[3:6], R @ rodrigues(d[6:9]), t + d[9:12]
        X = CORNERS[:len(v)] @ Qd.T + cd
        p = ((X @ Rd.T + td) - o) @ A.T
        e = p - v * (np.sum(v * p, 1) / np.sum(v * v, 1))[:, None]
        return e / np.linalg.norm(p, axis=1)[:, None]

    J = np.zeros((len(v), 3, 12))
    for k in range(12):
        d = np.zeros(12)
        d[k] = h
        J[:, :, k] = (res(d) - res(-d)) / (2 * h)
    return J
