"""Helpers of the per-tag pose tests: ground truth of rendered tags, exact projections of random poses, error metrics and the
GPU-vs-restatement comparison with its borderline rules (DESIGN.md §Per-tag pose)."""
import math

import numpy as np

import np_tag_pose as T

# GPU against the numpy restatement (measured maxima 2.5e-12, 1.4e-12, 1.8e-11: DESIGN.md §Per-tag pose)
TOL_R = 1e-9          # max |R_gpu - R_np| entry
TOL_T = 1e-9          # max |t_gpu - t_np| / max(1, |t|)
TOL_ERR = 1e-9        # |err_gpu - err_np| / max(err, 1e-12)
# rendered frames against the truth (bounds from the measured distribution: DESIGN.md §Per-tag pose)
TRUTH_T_REL = 0.08            # |t - t_true| / |t_true|, every matched detection (measured max 0.051)
TRUTH_ROT_BEST_DEG = 40.0     # the better of pose and alternative, every detection (measured max 34: small near-frontal tags)
TRUTH_ROT_MEDIAN_DEG = 1.0    # median rotation error of the pose itself, synth.render frames (measured 0.30)
TRUTH_ROT_P90_DEG = 3.0       # 90th percentile of the same (measured 1.1)


def truth_errors(rec, R, t):
    """(rotation error of the pose in degrees, of the better of pose and alternative, relative translation error)."""
    e = rot_deg(rec["R"], R)
    ea = rot_deg(rec["R_alt"], R) if rec["has_alt"] else e
    return e, min(e, ea), float(np.linalg.norm(rec["t"] - t) / np.linalg.norm(t))


def match_synth(d_corners, d_id, truth, tol=3.0):
    """The truth tag a detection is of: same id, every corner within tol pixels; None for a false positive."""
    for tr in truth:
        if tr["id"] == d_id and np.abs(tr["corners"] - d_corners).max() <= tol:
            return tr
    return None


def synth_truth(H, w, h, tagsize):
    """(R, t) of a synth.render tag: K^-1 H = [r1 r2 T] with K = [[w,0,w/2],[0,w,h/2],[0,0,1]]; t = s T."""
    K = np.array([[w, 0, w / 2.0], [0, w, h / 2.0], [0, 0, 1.0]])
    M = np.linalg.solve(K, H)
    r1, r2 = M[:, 0], M[:, 1]
    return np.stack([r1, r2, np.cross(r1, r2)], 1), 0.5 * tagsize * M[:, 2]


def view_truths(layout, robot_xy_yaw, r2c):
    """{tag id: (R, t)} of the field tags of a scenes.render_view frame, in the camera frame, for tag-local corners
    (0, -S, -S), (0, S, -S), (0, S, S), (0, -S, S) <-> object corners s(-1,1,0), s(1,1,0), s(1,-1,0), s(-1,-1,0) (the same map
    render_view draws with)."""
    from chalkydri_amd import scenes
    x, y, yaw = robot_xy_yaw
    Rwr = scenes.euler_to_mat(0, 0, yaw)
    Rrc, trc = scenes.solver_camera_transform(r2c["x"], r2c["y"], r2c["z"], r2c["roll"], r2c["pitch"], r2c["yaw"])
    Rcw = Rrc @ Rwr.T
    tcw = trc - Rcw @ np.array([x, y, 0.0])
    out = {}
    for t in layout["tags"]:
        tr, q = t["pose"]["translation"], t["pose"]["rotation"]["quaternion"]
        Rtw = scenes.quat_to_mat([q["W"], q["X"], q["Y"], q["Z"]])
        r1, r2 = Rcw @ Rtw @ np.array([0, 1.0, 0]), Rcw @ Rtw @ np.array([0, 0, -1.0])
        out[t["ID"]] = (np.stack([r1, r2, np.cross(r1, r2)], 1), Rcw @ np.array([tr["x"], tr["y"], tr["z"]]) + tcw)
    return out


def rot_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return math.degrees(math.acos(max(-1.0, min(1.0, c))))


def rot(axis, a):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def random_pose(rng, dmin=0.5, dmax=8.0, tilt_max_deg=70.0):
    """Tag at distance dmin..dmax inside a +-17 x 11 degree cone, tilted 0..tilt_max about an in-plane axis, any roll."""
    d = rng.uniform(dmin, dmax)
    tilt = math.radians(rng.uniform(0, tilt_max_deg))
    ax = np.array([rng.normal(), rng.normal(), 0.0])
    R = rot(ax, tilt) @ rot([0, 0, 1.0], rng.uniform(-math.pi, math.pi))
    dirn = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), 1.0])
    return R, dirn / np.linalg.norm(dirn) * d


def project(R, t, s, cam):
    """Pixel corners of the tag (R, t) of half-size s through a pinhole (fx, fy, cx, cy, ...)."""
    fx, fy, cx, cy = cam[:4]
    P = T.object_points(s) @ R.T + t
    return np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], 1)


def records_of(gpu):
    """ctypes TagPose records -> dicts with the np_tag_pose field names."""
    out = []
    for r in gpu:
        out.append({"id": r.id, "family": r.family, "valid": r.valid, "has_alt": r.has_alt,
                    "R": np.array(r.R[:]).reshape(3, 3), "t": np.array(r.t[:]), "err": r.err,
                    "R_alt": np.array(r.R_alt[:]).reshape(3, 3), "t_alt": np.array(r.t_alt[:]), "err_alt": r.err_alt,
                    "H": np.array(r.H[:]).reshape(3, 3)})
    return out


def borderline(info):
    """A case whose has_alt may legitimately differ between two correct implementations: a root within 1e-9 of the
    0.1 rad cut, or a derivative test within rounding of 0."""
    for x, dP, dist, P in (info or {}).get("roots", []):
        scale = max(abs(c) for c in P) * max(1.0, abs(x)) ** 3
        if abs(dist - T.MIN_DISTINCT_BETA) < 1e-9 or abs(dP) <= 1e-9 * scale:
            return True
    return False


def _close(a, b):
    dR = float(np.abs(a[0] - b[0]).max())
    dt = float(np.abs(a[1] - b[1]).max() / max(1.0, np.linalg.norm(b[1])))
    de = abs(a[2] - b[2]) / max(abs(b[2]), 1e-12)
    return dR, dt, de


def compare(gpu, ref, infos, stats=None):
    """Mismatch descriptions of GPU records against np_tag_pose records (lists of dicts).  stats (a dict) collects the
    largest deviations and the counts of borderline and tie cases."""
    bad = []
    st = stats if stats is not None else {}
    for k in ("dR", "dt", "derr"):
        st.setdefault(k, 0.0)
    for k in ("n", "borderline", "ties", "alts"):
        st.setdefault(k, 0)
    for i, (g, r) in enumerate(zip(gpu, ref)):
        st["n"] += 1
        if (g["id"], g["family"], g["valid"]) != (r["id"], r["family"], r["valid"]):
            bad.append((i, "id/family/valid", g["valid"], r["valid"]))
            continue
        if not g["valid"]:
            continue
        if not np.allclose(g["H"], r["H"], rtol=1e-9, atol=1e-9):
            bad.append((i, "H", float(np.abs(g["H"] - r["H"]).max())))
        border = borderline(infos.get(i)) if infos is not None else False
        if g["has_alt"] != r["has_alt"]:
            if border:
                st["borderline"] += 1
                continue
            bad.append((i, "has_alt", g["has_alt"], r["has_alt"]))
            continue
        first = _close((g["R"], g["t"], g["err"]), (r["R"], r["t"], r["err"]))
        if g["has_alt"]:
            st["alts"] += 1
            second = _close((g["R_alt"], g["t_alt"], g["err_alt"]), (r["R_alt"], r["t_alt"], r["err_alt"]))
            if max(first[0], first[1]) > TOL_R and abs(r["err"] - r["err_alt"]) <= 1e-9 * max(r["err"], 1e-12):
                # a tie of the two errors: the order may differ
                sw1 = _close((g["R"], g["t"], g["err"]), (r["R_alt"], r["t_alt"], r["err_alt"]))
                sw2 = _close((g["R_alt"], g["t_alt"], g["err_alt"]), (r["R"], r["t"], r["err"]))
                if max(sw1 + sw2) <= TOL_R:
                    st["ties"] += 1
                    first, second = sw1, sw2
            for a, b in zip(("dR", "dt", "derr"), second):
                st[a] = max(st[a], b)
            if second[0] > TOL_R or second[1] > TOL_T or second[2] > TOL_ERR:
                bad.append((i, "alt", second))
        for a, b in zip(("dR", "dt", "derr"), first):
            st[a] = max(st[a], b)
        if first[0] > TOL_R or first[1] > TOL_T or first[2] > TOL_ERR:
            bad.append((i, "pose", first))
    return bad


def np_poses(dets, cam, tagsizes, n_iters=50):
    """np_tag_pose on ck_detection_t records; returns (records, infos)."""
    infos = {}
    corners = np.array([[[d.p[k][0], d.p[k][1]] for k in range(4)] for d in dets]).reshape(-1, 4, 2)
    ref = T.estimate_tag_poses(corners, [d.family for d in dets], [d.id for d in dets], cam, tagsizes, n_iters, infos)
    return ref, infos
