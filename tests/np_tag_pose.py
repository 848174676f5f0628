"""float64 numpy restatement of the per-tag pose contract (DESIGN.md §Per-tag pose; AprilTag-3's estimate_tag_pose), step for
step as chalkydri_amd/csrc/k_tagpose.hip runs it, including the same root finder (no np.roots).  numpy.linalg.svd stands in for
the kernel's Jacobi SVD: the nearest rotation U diag(1, 1, det(U V^T)) V^T does not depend on which SVD produced it.  Test
infrastructure only: the GPU is compared with it."""
import math

import numpy as np

POLY_MAX_ROOT = 1000.0
MIN_DISTINCT_BETA = 0.1
SINGULAR_G = 1e-12
SQUARE = np.array([[-1.0, 1.0], [1.0, 1.0], [1.0, -1.0], [-1.0, -1.0]])   # object corners / s, in detection order
M1 = np.array([[0.0, 0, 2], [0, 0, 0], [-2, 0, 0]])
M2 = np.diag([-1.0, 1.0, -1.0])


def object_points(s):
    return np.array([[-s, s, 0.0], [s, s, 0.0], [s, -s, 0.0], [-s, -s, 0.0]])


def undistort(cam, u, v):
    """(x, y, converged) arrays: the fixed-point iteration of the reference's OpenCVModel5 unproject, per point (k_sqpnp.hip)."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    u, v = np.asarray(u, float), np.asarray(v, float)
    with np.errstate(all="ignore"):
        xd, yd = (u - cx) / fx, (v - cy) / fy
        x, y = xd.copy(), yd.copy()
        conv = np.zeros(x.shape, bool)
        for _ in range(50):
            act = ~conv
            if not act.any():
                break
            xa, ya = x[act], y[act]
            r2 = xa * xa + ya * ya
            radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            dx = 2.0 * p1 * xa * ya + p2 * (r2 + 2.0 * xa * xa)
            dy = p1 * (r2 + 2.0 * ya * ya) + 2.0 * p2 * xa * ya
            nx, ny = (xd[act] - dx) / radial, (yd[act] - dy) / radial
            ex, ey = nx - xa, ny - ya
            x[act], y[act] = nx, ny
            conv[act] = ex * ex + ey * ey < 1e-24
    return x, y, conv & np.isfinite(x) & np.isfinite(y)


def square_homography(x, y):
    """G (3x3, up to scale) with G (S_i, 1) ~ (x_i, y_i, 1), or None (Heckbert's unit-square map composed with
    (u, v) = ((X + 1) / 2, (1 - Y) / 2))."""
    with np.errstate(all="ignore"):
        sx, sy = x[0] - x[1] + x[2] - x[3], y[0] - y[1] + y[2] - y[3]
        dx1, dx2, dy1, dy2 = x[1] - x[2], x[3] - x[2], y[1] - y[2], y[3] - y[2]
        den = dx1 * dy2 - dx2 * dy1
        if den == 0.0:
            return None
        g, hh = (sx * dy2 - dx2 * sy) / den, (dx1 * sy - sx * dy1) / den
        a, b, c = x[1] - x[0] + g * x[1], x[3] - x[0] + hh * x[3], x[0]
        d, e, f = y[1] - y[0] + g * y[1], y[3] - y[0] + hh * y[3], y[0]
        G = np.array([[0.5 * a, -0.5 * b, 0.5 * (a + b) + c],
                      [0.5 * d, -0.5 * e, 0.5 * (d + e) + f],
                      [0.5 * g, -0.5 * hh, 0.5 * (g + hh) + 1.0]])
    return G if np.all(np.isfinite(G)) else None


def nearest_rotation(M):
    """U diag(1, 1, det(U V^T)) V^T, batched over leading axes."""
    U, _, Vt = np.linalg.svd(M)
    d = np.sign(np.linalg.det(U @ Vt))
    d[d == 0] = 1.0
    U = U.copy()
    U[..., :, 2] *= d[..., None]
    return U @ Vt


def calc_F(v):
    """v v^T / v^T v, batched: v [..., 3] -> [..., 3, 3]."""
    return v[..., :, None] * v[..., None, :] / np.sum(v * v, -1)[..., None, None]


def orthogonal_iteration(p, F, Minv, R, n_iters):
    """Batched over N problems: p [N,4,3], F [N,4,3,3], Minv [N,3,3], R [N,3,3] -> (R, t, err); no early exit, t of the last
    step predates its rotation update."""
    R = R.copy()
    t = np.zeros(R.shape[:-2] + (3,))
    err = np.zeros(R.shape[:-2])
    pm = p.mean(1)
    for _ in range(n_iters):
        Rp = np.einsum("nij,nkj->nki", R, p)
        acc = np.einsum("nkij,nkj->nki", F, Rp) - Rp
        t = np.einsum("nij,nj->ni", Minv, acc.sum(1) * 0.25)
        q = np.einsum("nkij,nkj->nki", F, Rp + t[:, None, :])
        qm = q.mean(1)
        M = np.einsum("nka,nkb->nab", q - qm[:, None, :], p - pm[:, None, :])
        R = nearest_rotation(M)
        w = np.einsum("nij,nkj->nki", R, p) + t[:, None, :]
        e = w - np.einsum("nkij,nkj->nki", F, w)
        err = np.sum(e * e, axis=(1, 2))
    return R, t, err


def horner(p, x):
    v = p[-1]
    for c in p[-2::-1]:
        v = v * x + c
    return v


def poly_roots(p):
    """Real roots in [-1000, 1000], ascending, of p[0] + p[1] x + ... (AprilTag-3's solve_poly_approx shape)."""
    D = len(p) - 1
    if D == 1:
        if p[1] == 0.0 or abs(p[0]) > POLY_MAX_ROOT * abs(p[1]):
            return []
        return [-p[0] / p[1]]
    pd = [(i + 1) * p[i + 1] for i in range(D)]
    dr = poly_roots(pd)
    out = []
    for i in range(len(dr) + 1):
        lo = -POLY_MAX_ROOT if i == 0 else dr[i - 1]
        hi = POLY_MAX_ROOT if i == len(dr) else dr[i]
        flo, fhi = horner(p, lo), horner(p, hi)
        if flo * fhi < 0:
            lower, upper = (lo, hi) if flo < fhi else (hi, lo)
            root = 0.5 * (lower + upper)
            dx_old = upper - lower
            dx = dx_old
            f, df = horner(p, root), horner(pd, root)
            for _ in range(100):
                if f == 0.0:
                    break
                if ((root - upper) * df - f) * ((root - lower) * df - f) > 0 or abs(2.0 * f) > abs(dx_old * df):
                    dx_old, dx = dx, 0.5 * (upper - lower)
                    root = lower + dx
                else:
                    dx_old, dx = dx, -f / df
                    root += dx
                if root == upper or root == lower:
                    break
                f, df = horner(p, root), horner(pd, root)
                if f > 0:
                    upper = root
                else:
                    lower = root
            out.append(root)
        elif fhi == 0.0:
            out.append(hi)
    return out


def ambiguity_frame(R, t):
    """(Rt, Rz, Rg, beta0) of §Second minimum."""
    th = t / math.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    e1 = np.array([1.0 - th[0] * th[0], -th[0] * th[1], -th[0] * th[2]])
    e1 = e1 / math.sqrt(e1 @ e1)
    e2 = np.cross(th, e1)
    Rt = np.stack([e1, e2, th])
    Rp = Rt @ R
    r31, r32 = Rp[2, 0], Rp[2, 1]
    h = math.sqrt(r31 * r31 + r32 * r32)
    if h < 1e-100:
        r31, r32, h = 1.0, 0.0, 1.0
    cz, sz = r31 / h, r32 / h
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    Rtr = Rp @ Rz
    sg, cg = -Rtr[0, 1], Rtr[1, 1]
    Rg = np.array([[cg, -sg, 0.0], [sg, cg, 0.0], [0.0, 0.0, 1.0]])
    return Rt, Rz, Rg, math.atan2(-Rtr[2, 0], Rtr[2, 2])


def quartic_coeffs(p, v, R, t):
    """(a0..a4, Rt, Rz, Rg, beta0): (1 + tau^2)^2 E(tau) = sum a_k tau^k along R(tau) = Rt^T Rg Rb(tau) Rz^T with the optimal
    translation; None when (I - mean F') cannot be inverted."""
    Rt, Rz, Rg, beta0 = ambiguity_frame(R, t)
    pp = p @ Rz            # rows: Rz^T p_i
    vp = v @ Rt.T          # rows: Rt v_i
    Fp = calc_F(vp)
    A = np.eye(3) - Fp.mean(0)
    if np.linalg.det(A) == 0.0:
        return None
    Gm = np.linalg.inv(A) * 0.25
    Mp = [pp @ Rg.T, pp @ (Rg @ M1).T, pp @ (Rg @ M2).T]          # [k][i] = Rg M_k p'_i
    b = [Gm @ (np.einsum("kij,kj->ki", Fp, m) - m).sum(0) for m in Mp]
    c = [(m + bk) - np.einsum("kij,kj->ki", Fp, m + bk) for m, bk in zip(Mp, b)]
    dot = lambda x, y: float(np.sum(x * y))
    a = (dot(c[0], c[0]), 2 * dot(c[0], c[1]), dot(c[1], c[1]) + 2 * dot(c[0], c[2]), 2 * dot(c[1], c[2]), dot(c[2], c[2]))
    return a, Rt, Rz, Rg, beta0


def R_of_tau(Rt, Rz, Rg, tau):
    den = 1.0 + tau * tau
    cb, sb = (1.0 - tau * tau) / den, (2.0 * tau) / den
    Rb = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    return Rt.T @ Rg @ Rb @ Rz.T


def second_minimum(p, v, R, t, info=None):
    """The seed R2 of the second run, or None (zero or several minima besides the first).  info (a dict) receives the roots,
    the derivative test values and the angle distances, for the borderline flags of the tests."""
    qc = quartic_coeffs(p, v, R, t)
    if qc is None:
        return None
    (a0, a1, a2, a3, a4), Rt, Rz, Rg, beta0 = qc
    P = [a1, 2 * a2 - 4 * a0, 3 * a3 - 3 * a1, 4 * a4 - 2 * a2, -a3]
    roots = poly_roots(P)
    kept = []
    for x in roots:
        dP = P[1] + x * (2.0 * P[2] + x * (3.0 * P[3] + x * (4.0 * P[4])))
        dist = abs(2.0 * math.atan(x) - beta0)
        if info is not None:
            info.setdefault("roots", []).append((x, dP, dist, P))
        if dP > 0.0 and dist > MIN_DISTINCT_BETA:
            kept.append(x)
    if len(kept) != 1:
        return None
    R2 = R_of_tau(Rt, Rz, Rg, kept[0])
    return R2 if np.all(np.isfinite(R2)) else None


def object_error(p, v, R, t):
    F = calc_F(v)
    w = p @ R.T + t
    e = w - np.einsum("kij,kj->ki", F, w)
    return float(np.sum(e * e))


def _invalid(det_id, family):
    z = np.zeros((3, 3))
    return {"id": det_id, "family": family, "valid": 0, "has_alt": 0, "R": z, "t": np.zeros(3), "err": 0.0,
            "R_alt": z, "t_alt": np.zeros(3), "err_alt": 0.0, "H": z}


def estimate_tag_poses(corners, families, ids, cam, tagsizes, n_iters=50, infos=None):
    """corners [N,4,2] pixels; families / ids [N]; cam = (fx, fy, cx, cy, k1, k2, p1, p2, k3); tagsizes by family.
    Returns one dict per detection with the ck_tag_pose_t fields (R, R_alt, H as 3x3)."""
    corners = np.asarray(corners, float).reshape(-1, 4, 2)
    N = len(corners)
    out = [_invalid(int(ids[i]), int(families[i])) for i in range(N)]
    prep = []   # (index, p, v, F, Minv, R0)
    for i in range(N):
        fam = int(families[i])
        if fam < 0 or fam >= len(tagsizes):
            continue
        s = 0.5 * float(tagsizes[fam])
        u, w = corners[i, :, 0], corners[i, :, 1]
        if not (np.all(np.isfinite(u)) and np.all(np.isfinite(w))):
            continue
        x, y, ok = undistort(cam, u, w)
        if not ok.all():
            continue
        G, H = square_homography(x, y), square_homography(u, w)
        if G is None or H is None:
            continue
        n1, n2, n3 = (math.sqrt(G[0, k] ** 2 + G[1, k] ** 2 + G[2, k] ** 2) for k in range(3))
        if not abs(np.linalg.det(G)) > SINGULAR_G * (n1 * n2 * n3):
            continue
        with np.errstate(all="ignore"):
            H = H / H[2, 2]
        if not np.all(np.isfinite(H)):
            continue
        lam = 1.0 / math.sqrt(n1 * n2)
        if G[2, 2] < 0.0:
            lam = -lam
        r1, r2 = lam * G[:, 0], lam * G[:, 1]
        M0 = np.stack([r1, r2, np.cross(r1, r2)], 1)
        t0 = s * lam * G[:, 2]
        if not (np.all(np.isfinite(M0)) and np.all(np.isfinite(t0))):
            continue
        R0 = nearest_rotation(M0[None])[0]
        v = np.stack([x, y, np.ones(4)], 1)
        F = calc_F(v)
        A = np.eye(3) - F.mean(0)
        if not np.all(np.isfinite(R0)) or np.linalg.det(A) == 0.0:
            continue
        Minv = np.linalg.inv(A)
        if not np.all(np.isfinite(Minv)):
            continue
        out[i]["H"] = H
        prep.append((i, object_points(s), v, F, Minv, R0))
    if not prep:
        return out
    idx = [q[0] for q in prep]
    P, V, F, Mi, R0 = (np.array([q[k] for q in prep]) for k in range(1, 6))
    R1, t1, e1 = orthogonal_iteration(P, F, Mi, R0, n_iters)
    seeds = []
    for j, i in enumerate(idx):
        info = {} if infos is not None else None
        ok1 = np.all(np.isfinite(R1[j])) and np.all(np.isfinite(t1[j])) and np.isfinite(e1[j])
        R2 = second_minimum(P[j], V[j], R1[j], t1[j], info) if ok1 else None
        if infos is not None:
            infos[i] = info
        seeds.append(R2)
    alt = [j for j, r in enumerate(seeds) if r is not None]
    R2s, t2s, e2s = {}, {}, {}
    if alt:
        a = np.array(alt)
        R2, t2, e2 = orthogonal_iteration(P[a], F[a], Mi[a], np.array([seeds[j] for j in alt]), n_iters)
        for k, j in enumerate(alt):
            R2s[j], t2s[j], e2s[j] = R2[k], t2[k], e2[k]
    for j, i in enumerate(idx):
        if not (np.all(np.isfinite(R1[j])) and np.all(np.isfinite(t1[j])) and np.isfinite(e1[j])):
            out[i]["H"] = np.zeros((3, 3))
            continue
        rec = out[i]
        has = j in R2s and np.all(np.isfinite(R2s[j])) and np.all(np.isfinite(t2s[j])) and np.isfinite(e2s[j])
        rec["valid"], rec["has_alt"] = 1, int(has)
        sols = [(R1[j], t1[j], float(e1[j]))]
        if has:
            sols.append((R2s[j], t2s[j], float(e2s[j])))
            if sols[1][2] < sols[0][2]:
                sols.reverse()
        rec["R"], rec["t"], rec["err"] = sols[0]
        if has:
            rec["R_alt"], rec["t_alt"], rec["err_alt"] = sols[1]
        else:
            rec["err_alt"] = math.inf
    return out
