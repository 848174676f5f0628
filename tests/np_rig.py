"""Numpy restatement of the camera-rig solver, written from the formulas and not from the C: numpy.linalg for the
SVD, the eigen-decomposition and the KKT solve.  It pins ck_rig_host.c, to which the device solver is pinned, and on the cases of
tests/rig_cases.py the device solver itself (tests/test_gpu_rig_cases.py): twin and kernels share their leaf arithmetic.

Frames: the unknown is world -> robot (R, t), p_robot = R X + t; camera c is mounted by robot_to_cam = (A_c, b_c), p_cam = A_c p_robot
+ b_c.  A bearing v of camera c is the ray u = A_c^T v through o_c = -A_c^T b_c; M = I - u u^T / u^T u;
E(R, t) = sum_i (R X_i + t - o_i)^T M_i (R X_i + t - o_i).  r = vec(R) column-major.
"""
import numpy as np

TAG_SIZE = 0.1651
S = TAG_SIZE / 2.0
CORNERS = np.array([[0, -S, -S], [0, S, -S], [0, S, S], [0, -S, S]], float)
CV_FROM_TAG = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], float).T   # a tag whose normal (local x) looks down the camera's -z


def quat_to_mat(q):
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def mat_to_quat(R):
    """(w, x, y, z) of a rotation matrix, by the largest of the four squared components."""
    K = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                  1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(K))
    s = 2 * np.sqrt(K[k])
    if k == 0:
        q = [s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif k == 1:
        q = [(R[2, 1] - R[1, 2]) / s, s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif k == 2:
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s]
    else:
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4]
    q = np.array(q)
    return q / np.linalg.norm(q)


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])


def random_rotation(rng):
    q = rng.normal(size=4)
    return quat_to_mat(q / np.linalg.norm(q))


def small_rotation(rng, amount):
    w = rng.uniform(-amount, amount, 3)
    a = np.linalg.norm(w)
    if a < 1e-12:
        return np.eye(3)
    k = w / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def nearest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        U = U.copy()
        U[:, 2] *= -1
        R = U @ Vt
    return R


# ---- the system ---------------------------------------------------------------------------------------------------------------
class System:
    """Everything of one step that does not depend on r.  cams: [(tags [(R, t)], bearings (4n, 3), (A, b))]."""

    def __init__(self, cams):
        X, U, O, cam_of = [], [], [], []
        self.mounts = [(np.asarray(A, float), np.asarray(b, float)) for _, _, (A, b) in cams]
        self.cam_tags = [len(tags) for tags, _, _ in cams]
        self.tag_centres = [t for tags, _, _ in cams for _, t in tags]
        for c, (tags, bearings, _) in enumerate(cams):
            A, b = self.mounts[c]
            bearings = np.asarray(bearings, float).reshape(-1, 3)
            assert len(bearings) == 4 * len(tags)
            for k, (R, t) in enumerate(tags):
                for j in range(4):
                    X.append(R @ CORNERS[j] + t)
                    U.append(A.T @ bearings[4 * k + j])
                    O.append(-A.T @ b)
                    cam_of.append(c)
        self.X, self.U, self.O, self.cam_of = np.array(X).reshape(-1, 3), np.array(U).reshape(-1, 3), np.array(O).reshape(-1, 3), np.array(cam_of, int)
        self.n = len(self.X)
        if self.n == 0:
            return
        self.centroid = self.X.mean(0)
        Q_rr, Q_rt, Q_tt = np.zeros((9, 9)), np.zeros((9, 3)), np.zeros((3, 3))
        q_r, q_t, q_0 = np.zeros(9), np.zeros(3), 0.0
        self.M = []
        for x, u, o in zip(self.X - self.centroid, self.U, self.O):
            M = np.eye(3) - np.outer(u, u) / (u @ u)
            L = np.kron(x.reshape(1, 3), np.eye(3))        # 3 x 9: L r = R x for r = vec(R) column-major
            Q_tt += M
            Q_rt += L.T @ M
            Q_rr += L.T @ M @ L
            q_r += L.T @ M @ o
            q_t += M @ o
            q_0 += o @ M @ o
            self.M.append(M)
        self.Q_rt, self.q_t = Q_rt, q_t
        self.Q_tt_inv = np.linalg.inv(Q_tt) if abs(np.linalg.det(Q_tt)) > 0 else np.zeros((3, 3))
        self.omega = Q_rr - Q_rt @ self.Q_tt_inv @ Q_rt.T
        self.g = q_r - Q_rt @ self.Q_tt_inv @ q_t
        self.c = q_0 - q_t @ self.Q_tt_inv @ q_t
        # Coplanar points (one tag, tags on one wall) with normal n leave R n free: Omega has the exact null space {vec(a n^T)}, whose
        # basis says nothing about the pose.  The starts then come from the complement: that space is moved to the top of the
        # spectrum by mu * sum_k v_k v_k^T, v_k = vec(e_k n^T), mu = trace(Q_rr).
        Xc = self.X - self.centroid
        w, V = np.linalg.eigh(Xc.T @ Xc)
        self.omega_starts = self.omega.copy()
        self.scatter_w = w                                  # (read-out only)
        self.coplanar = bool(w[0] <= 1e-12 * w[2])
        if self.coplanar:
            for k in range(3):
                v = np.kron(V[:, 0], np.eye(3)[k])
                self.omega_starts += np.trace(Q_rr) * np.outer(v, v)

    def energy(self, r):
        return r @ self.omega @ r - 2 * self.g @ r + self.c

    def translation(self, r):
        R = r.reshape(3, 3).T
        return self.Q_tt_inv @ (self.q_t - self.Q_rt.T @ r) - R @ self.centroid

    def in_front(self, r):
        R, t = r.reshape(3, 3).T, self.translation(r)
        P = self.X @ R.T + t
        return all((self.mounts[c][0] @ p + self.mounts[c][1])[2] > 0 for p, c in zip(P, self.cam_of))

    def residuals(self, r):
        """squared point-to-ray distance of every point at the returned pose (polar(R(r)), t(r))"""
        R, t = nearest_rotation(r.reshape(3, 3).T), self.translation(r)
        D = self.X @ R.T + t - self.O
        return np.array([(M @ d) @ (M @ d) for d, M in zip(D, self.M)])      # d^T M d = |M d|^2: M is a projector


def constraints(r):
    c1, c2, c3 = r[0:3], r[3:6], r[6:9]
    h = np.array([c1 @ c1 - 1, c2 @ c2 - 1, c3 @ c3 - 1, c1 @ c2, c1 @ c3, c2 @ c3])
    J = np.zeros((6, 9))
    J[0, 0:3] = 2 * c1; J[1, 3:6] = 2 * c2; J[2, 6:9] = 2 * c3
    J[3, 0:3] = c2; J[3, 3:6] = c1; J[4, 0:3] = c3; J[4, 6:9] = c1; J[5, 3:6] = c3; J[5, 6:9] = c2
    return h, J


def sqp(sys, r, max_iter, tol_sq):
    r = r.copy()
    for _ in range(max_iter):
        h, J = constraints(r)
        lhs = np.zeros((15, 15))
        lhs[:9, :9] = sys.omega; lhs[:9, 9:] = J.T; lhs[9:, :9] = J
        rhs = np.concatenate([-(sys.omega @ r - sys.g), -h])
        try:
            d = np.linalg.solve(lhs, rhs)[:9]
        except np.linalg.LinAlgError:
            break
        r += d
        if d @ d < tol_sq:
            break
    return r


def penalised(sys, r, gyro, sign_change_error):
    return sys.energy(r) + sign_change_error * max(0.0, 1.0 - (r[0] * np.cos(gyro) + r[3] * np.sin(gyro)))


def pick(sys, cands, gyro, sign_change_error, trace=None):
    """the first candidate, by penalised energy, with every point in front of its own camera"""
    ordered = sorted(cands, key=lambda r: penalised(sys, r, gyro, sign_change_error))
    if trace is not None:                                   # read-out: every candidate in penalised order with its verdict, the winner
        trace["candidates"] = [{"penalised": float(penalised(sys, r, gyro, sign_change_error)), "energy": float(sys.energy(r)),
                                "in_front": bool(sys.in_front(r))} for r in ordered]
        trace["winner"] = next((k for k, c in enumerate(trace["candidates"]) if c["in_front"]), None)
    for r in ordered:
        if sys.in_front(r):
            return r
    return None


def _branch(raw, lo, hi):
    return "lo" if raw < lo else ("hi" if raw > hi else "mid")


def finish(sys, r, gyro, trace=None):
    """the result record of the chosen r"""
    R, t = r.reshape(3, 3).T, sys.translation(r)
    res = sys.residuals(r)
    E = sum(res[sys.cam_of == c].sum() for c in range(len(sys.cam_tags)))   # E as the cost's own sum at the returned pose
    rot0 = nearest_rotation(R).T
    pos0 = -rot0 @ t
    n_tags = sum(sys.cam_tags)
    rms = np.sqrt(max(E, 0.0) / (4 * n_tags))
    if rms > 0.1:
        std = np.full(3, np.finfo(float).max)
    else:
        m = 1 + np.linalg.norm(t) / TAG_SIZE
        xy = np.clip(rms * m / np.sqrt(n_tags) * 5.0, 0.01, 10.0)
        th = np.clip(rms / TAG_SIZE * m / np.sqrt(n_tags) * 2.0, 0.05, np.pi)
        std = np.array([xy, xy, th])
    tc = np.mean(sys.tag_centres, 0)
    d = (gyro - np.arctan2(rot0[1, 0], rot0[0, 0]) + np.pi) % (2 * np.pi) - np.pi
    w = np.clip(abs(np.degrees(d)) / 30.0, 0, 1)
    w = w * w * (3 - 2 * w)
    Rz = rot_z(d * w)
    rot, pos = Rz @ rot0, tc + Rz @ (pos0 - tc)
    yaw = np.arctan2(rot[1, 0], rot[0, 0]) if abs(rot[2, 0]) < 1 else 0.0
    cam_rms = [np.sqrt(max(res[sys.cam_of == c].sum(), 0.0) / (4 * k)) if k else 0.0 for c, k in enumerate(sys.cam_tags)]
    if trace is not None:                                   # read-out: the yaw pivot, the branches of the standard deviations, the polar step
        mult = 1 + np.linalg.norm(t) / TAG_SIZE
        U, _, Vt = np.linalg.svd(R)
        trace.update(yaw_delta=float(d), yaw_weight=float(w), vision_yaw=float(np.arctan2(rot0[1, 0], rot0[0, 0])), rms=float(rms),
                     std_branch=("untrusted",) if rms > 0.1 else (_branch(rms * mult / np.sqrt(n_tags) * 5.0, 0.01, 10.0),
                                                                  _branch(rms / TAG_SIZE * mult / np.sqrt(n_tags) * 2.0, 0.05, np.pi)),
                     polar_flip=bool(np.linalg.det(U @ Vt) < 0))
    return {"rot": rot, "pos": pos, "std": std, "yaw": yaw, "energy": E, "n_tags": n_tags, "cam_tags": list(sys.cam_tags),
            "cam_rms": cam_rms, "r": r, "t": t}


def solve_rig(cams, gyro, sign_change_error=600.0, max_iter=15, tol_sq=1e-16, trace=None):
    """The solver: SQPnP's six starts (the three smallest eigenvectors of Omega, both signs, through the nearest rotation; for
    coplanar points the three smallest outside Omega's exact null space).  `trace`: a dict that receives the read-out (the coplanar
    flag and the scatter's eigenvalue ratio, the candidates in penalised order with their in-front verdicts, the winner's index, the
    yaw delta and its smoothstep weight, rms and the branches of the standard deviations); it adds output only."""
    sys = System(cams)
    if sys.n < 3:
        return None
    if trace is not None:
        trace.update(coplanar=sys.coplanar, planar_ratio=float(sys.scatter_w[0] / sys.scatter_w[2]) if sys.scatter_w[2] > 0 else 0.0)
    w, V = np.linalg.eigh(sys.omega_starts)
    order = np.argsort(w, kind="stable")
    cands = []
    for i in order[:3]:
        for sign in (-1.0, 1.0):
            start = nearest_rotation((V[:, i] * sign).reshape(3, 3).T).T.reshape(9)
            cands.append(sqp(sys, start, max_iter, tol_sq))
    r = pick(sys, cands, gyro, sign_change_error, trace)
    return None if r is None else finish(sys, r, gyro, trace)


def many_start_reference(cams, gyro, truth_R, rng, n_starts=60, iters=100, sign_change_error=600.0, tol_sq=1e-16):
    """n_starts random rotations plus the truth as starts, `iters` iterations each: the global minimum to compare the six starts with."""
    sys = System(cams)
    starts = [random_rotation(rng) for _ in range(n_starts)] + [np.asarray(truth_R, float)]
    cands = [sqp(sys, R.T.reshape(9), iters, tol_sq) for R in starts]
    cands = [r for r in cands if np.all(np.isfinite(r)) and np.abs(constraints(r)[0]).max() < 1e-9]
    r = pick(sys, cands, gyro, sign_change_error)
    return None if r is None else finish(sys, r, gyro)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def make_rig(rng, n_cams=None, noise=0.0, tags_per_cam=(0, 3), gyro_noise=0.0, mount_translation=0.4):
    """A random rig: n_cams cameras (1..4 when None), mounts within +-mount_translation m and any rotation, tags_per_cam tags per
    camera (at least one in total) 1..5 m in front of their camera, bearing noise in normalised image coordinates.  Returns
    (cams as System takes them, gyro, truth {"rot": world <- robot, "pos", "R": world -> robot})."""
    n_cams = int(rng.integers(1, 5)) if n_cams is None else n_cams
    yaw = rng.uniform(-np.pi, np.pi)
    Rwr, twr = rot_z(yaw), np.array([rng.uniform(2, 14), rng.uniform(1, 7), 0.0])
    counts = [int(rng.integers(tags_per_cam[0], tags_per_cam[1] + 1)) for _ in range(n_cams)]
    if sum(counts) == 0:
        counts[int(rng.integers(n_cams))] = max(1, tags_per_cam[0])
    cams = []
    for c in range(n_cams):
        A = random_rotation(rng)                                   # cam <- robot
        b = -A @ rng.uniform(-mount_translation, mount_translation, 3)     # the camera sits at -A^T b in the robot frame
        tags, bearings = [], []
        for _ in range(counts[c]):
            z = rng.uniform(1.0, 5.0)
            pc = np.array([rng.uniform(-0.4, 0.4) * z, rng.uniform(-0.3, 0.3) * z, z])
            Rtc = small_rotation(rng, 0.5) @ CV_FROM_TAG           # cam <- tag
            Rcw = A @ Rwr.T                                        # cam <- world
            tcw = b - Rcw @ twr
            Rtw, ttw = Rcw.T @ Rtc, Rcw.T @ (pc - tcw)
            tags.append((Rtw, ttw))
            pts = (Rtw @ CORNERS.T).T + ttw
            cam_pts = pts @ Rcw.T + tcw
            xy = cam_pts[:, :2] / cam_pts[:, 2:3]
            if noise > 0:
                xy = xy + rng.normal(0, noise, xy.shape)
            v = np.concatenate([xy, np.ones((4, 1))], 1)
            bearings.append(v / np.linalg.norm(v, axis=1, keepdims=True))
        cams.append((tags, np.concatenate(bearings) if bearings else np.zeros((0, 3)), (A, b)))
    gyro = yaw + (rng.normal(0, gyro_noise) if gyro_noise > 0 else 0.0)
    return cams, gyro, {"rot": Rwr, "pos": twr, "R": Rwr.T, "yaw": yaw}
