"""Named, seeded cases of the parity tests of the rig pose solvers (k_rig and k_rig_robust, chalkydri_amd/csrc/k_rigpnp.hip; DESIGN.md
§4k, §4n): tests/test_gpu_rig_cases.py on the device, tests/test_rig_cases_host.py for the proof that every case reaches the edge it
is named for and for the twin against the restatement.  Nothing here touches the GPU.

A case is ONE call: one n_cams, at most 8 steps, plain (ck_rig_solve_*) or robust (ck_rig_solve_robust_*).  It is a dict:
    name, n_cams, edge (what it is built for), steps [cams as np_rig.System takes them], gyro [per step],
    robust (None: the plain call; else the keyword arguments of RobustParams / np_rig_robust.solve_robust),
    planted (robust: per step the planted mask of every camera), twin_only (judged against the host twin alone).
The scenes are built as np_rig.make_rig builds them (a true pose, mounts, tags in front of their camera, bearings by projection);
then the named deviation is applied.  Every construction is seeded.

restated(name) solves every step with the numpy restatement (tests/np_rig.py, tests/np_rig_robust.py) with its read-out, and again
on 8 copies whose bearings and tag translations are multiplied by 1 +- 2^-50 (seeded signs): the discrete results of the 9 solves
have to be identical ("stable"), and the largest change of a continuous one is the step's conditioning figure kappa, a property of
the reference alone.  The bound of a continuous comparison against the restatement is max(1e-9, 64 kappa): 1e-9 is the project's
line (TOL of tests/test_gpu_rig.py and tests/test_rig_host.py), the factor 64 is for the different but legitimate summation orders
and factorisations of the two sides."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import np_rig as N  # noqa: E402
import np_rig_robust as NR  # noqa: E402

TOL = 1e-9                      # tests/test_gpu_rig.py's TOL
KAPPA_FACTOR = 64.0
EMPTY = np.zeros((0, 3))
DBL_MAX = np.finfo(float).max


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def robot(rng, yaw=None):
    """the true pose as np_rig.make_rig draws it: (yaw, world <- robot rotation, position)"""
    yaw = rng.uniform(-np.pi, np.pi) if yaw is None else yaw
    return yaw, N.rot_z(yaw), np.array([rng.uniform(2, 14), rng.uniform(1, 7), 0.0])


def truth_of(yaw, Rwr, twr):
    return {"rot": Rwr, "pos": twr, "R": Rwr.T, "yaw": yaw}


def mount(rng, translation=0.4):
    A = N.random_rotation(rng)                                   # cam <- robot
    return A, -A @ rng.uniform(-translation, translation, 3)


def cam_from_world(A, b, Rwr, twr):
    Rcw = A @ Rwr.T
    return Rcw, b - Rcw @ twr


def tag_at(rng, A, b, Rwr, twr, z, tilt=0.5):
    """the world pose of a tag z m down the axis of camera (A, b), within np_rig.make_rig's field of view; z < 0: behind the camera"""
    pc = np.array([rng.uniform(-0.4, 0.4) * z, rng.uniform(-0.3, 0.3) * z, z])
    Rcw, tcw = cam_from_world(A, b, Rwr, twr)
    return Rcw.T @ (N.small_rotation(rng, tilt) @ N.CV_FROM_TAG), Rcw.T @ (pc - tcw)


def project(tags, A, b, Rwr, twr, noise=None):
    """the bearings of the tags' corners in camera (A, b) by projection (through the centre for a point behind it: the line is the
    same); noise [n][4][2] is added in normalised image coordinates"""
    Rcw, tcw = cam_from_world(A, b, Rwr, twr)
    out = []
    for k, (R, t) in enumerate(tags):
        pc = ((R @ N.CORNERS.T).T + t) @ Rcw.T + tcw
        xy = pc[:, :2] / pc[:, 2:3]
        if noise is not None:
            xy = xy + noise[k]
        v = np.concatenate([xy, np.ones((4, 1))], 1)
        out.append(v / np.linalg.norm(v, axis=1, keepdims=True))
    return np.concatenate(out) if out else EMPTY.copy()


def scene(rng, counts, noise=0.0, depth=(1.0, 5.0), depths=None, translation=0.4, yaw=None):
    """np_rig.make_rig with the number of tags of every camera given: counts[c] tags for camera c at a depth drawn from `depth`, or
    taken in turn from `depths`.  Returns (cams, true yaw, truth)."""
    yaw, Rwr, twr = robot(rng, yaw)
    cams = []
    for n in counts:
        A, b = mount(rng, translation)
        tags = [tag_at(rng, A, b, Rwr, twr, rng.uniform(*depth) if depths is None else depths[k % len(depths)]) for k in range(n)]
        nz = rng.normal(0, 1, (n, 4, 2)) * noise
        cams.append((tags, project(tags, A, b, Rwr, twr, nz if noise > 0 else None), (A, b)))
    return cams, yaw, truth_of(yaw, Rwr, twr)


def wall_scene(rng, counts, noise=0.0, lift=None):
    """All the tags of all the cameras on one wall 2-4 m from the robot, the cameras looking at it; lift = (camera, tag, d): that tag
    is pushed d m off the wall along its normal."""
    yaw, Rwr, twr = robot(rng)
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)                                       # the wall's normal, towards the robot
    p0 = twr - n * rng.uniform(2.0, 4.0)
    e1 = np.cross(n, [0.0, 0.0, 1.0] if abs(n[2]) < 0.9 else [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    cams = []
    for c, cnt in enumerate(counts):
        x = np.cos(a := rng.uniform(0, 2 * np.pi)) * e1 + np.sin(a) * e2
        Rlook = np.array([x, np.cross(-n, x), -n])               # cam <- world, the axis against the wall's normal
        Rcw = N.small_rotation(rng, 0.3) @ Rlook
        A = Rcw @ Rwr
        b = -A @ rng.uniform(-0.4, 0.4, 3)
        centre = Rwr @ (-A.T @ b) + twr
        tags = []
        for k in range(cnt):
            d = Rcw.T @ np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), 1.0])
            t = centre + d * (((p0 - centre) @ n) / (d @ n))
            s = rng.uniform(0, 2 * np.pi)
            Rt = np.array([n, np.cos(s) * e1 + np.sin(s) * e2, np.cross(n, np.cos(s) * e1 + np.sin(s) * e2)]).T
            if lift is not None and lift[:2] == (c, k):
                t = t + lift[2] * n
            tags.append((Rt, t))
        nz = rng.normal(0, 1, (cnt, 4, 2)) * noise
        cams.append((tags, project(tags, A, b, Rwr, twr, nz if noise > 0 else None), (A, b)))
    return cams, yaw, truth_of(yaw, Rwr, twr)


def with_noise(cams, truth, noise, scale, only=None):
    """cams with the bearings projected again under scale * noise (noise[c]: [n][4][2]); only = (camera, tag): that tag's alone"""
    out = []
    for c, (tags, _, (A, b)) in enumerate(cams):
        nz = noise[c] * scale
        if only is not None:
            keep = np.zeros(len(tags))
            if only[0] == c:
                keep[only[1]] = 1.0
            nz = noise[c] * (keep * scale + (1 - keep))[:, None, None]
        out.append((tags, project(tags, A, b, truth["rot"], truth["pos"], nz), (A, b)))
    return out


def tune(build, figure, target, start, power=1.0, iters=6):
    """the scale s at which figure(build(s)) is the target, for a figure that grows like s^power: a fixed number of fixed-point
    steps, so the construction is deterministic (the host test asserts where it landed)"""
    s = start
    for _ in range(iters):
        s *= (target / figure(build(s))) ** (1.0 / power)
    return s


def empty_like(cams):
    return [([], EMPTY.copy(), m) for _, _, m in cams]


def emptied(cams, keep):
    """cams with only the cameras in `keep` seeing anything"""
    return [cam if c in keep else ([], EMPTY.copy(), cam[2]) for c, cam in enumerate(cams)]


def compact(cams):
    """(the cameras that see a tag, their indices)"""
    idx = [c for c, (tags, _, _) in enumerate(cams) if len(tags)]
    return [cams[c] for c in idx], idx


def planted_scene(rng, cams, truth, where, kind="id"):
    masks = [0] * len(cams)
    for c, t in where:
        cams = NR.plant(rng, cams, truth, c, t, kind)
        masks[c] |= 1 << t
    return cams, masks


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def _case(name, n_cams, edge, steps, gyro, robust=None, planted=None, twin_only=False, **more):
    assert len(steps) == len(gyro) <= 8 and all(len(s) == n_cams for s in steps)
    c = {"name": name, "n_cams": n_cams, "edge": edge, "steps": steps, "gyro": [float(g) for g in gyro], "robust": robust,
         "planted": planted, "twin_only": twin_only}
    c.update(more)
    return c


ONE_CAMERA_COUNTS = (15, 16, 17, 31, 32, 33, 64)
FULL_PLANTED = ((0, 0), (0, 63), (1, 0), (1, 63), (2, 0), (3, 63), (4, 0), (7, 63))      # global tags 0, 63, 64, 127, 128, 255, 256, 511
BIT63_PLANTED = ((1, 0), (1, 63), (0, 63))
GYRO_A = (0.0, 10.0, 29.9, 30.0, 31.0, 90.0, 179.0, 180.0)
GYRO_B = (-10.0, -29.9, -30.0, -31.0, -90.0, -179.0)
NEAR_LIFTS = (1e-9, 1e-7, 1e-5, 1e-3, 1e-1)
STD_TARGETS = (None, 2e-3, 0.03, 0.09, 0.11)          # rms (m) of the steps of std_branches; None: no noise
CHEIRALITY_SECOND_SEEDS = (1, 2, 3)
CHEIRALITY_NONE_SEED = 0
FIRST_PASS_SEED = 0
ALL_OUTLIERS_SEEDS = (12, 20, 25, 0)                          # (the last one also finds no candidate in front on the first pass)


def _count_one_camera(robust):
    rng = np.random.default_rng(5101)
    steps, gyro, planted = [], [], []
    for n in ONE_CAMERA_COUNTS:
        cams, yaw, truth = scene(rng, [n], noise=1e-3)
        if robust:
            cams, m = planted_scene(rng, cams, truth, [(0, n - 1)])
            planted.append(m)
        steps.append(cams)
        gyro.append(yaw + rng.normal(0, 0.02))
    if robust:                                                    # and a clean step of 64 tags: the plain record, byte for byte
        cams, yaw, _ = scene(rng, [64], noise=1e-3)
        steps.append(cams); gyro.append(yaw); planted.append([0])
    return steps, gyro, planted


def _sized(seed, counts, noise, where, robust, extra=None):
    rng = np.random.default_rng(seed)
    cams, yaw, truth = scene(rng, counts, noise=noise)
    clean = cams
    steps, gyro, planted = [clean], [yaw + rng.normal(0, 0.02)], [[0] * len(counts)]
    if robust:
        cams, m = planted_scene(rng, cams, truth, where)
        steps, gyro, planted = [cams, clean], [gyro[0], gyro[0]], [m, planted[0]]
    elif extra is not None:
        more, yaw2, _ = scene(rng, extra, noise=noise)
        steps.append(more); gyro.append(yaw2)
    return steps, gyro, planted


def _sparse():
    rng = np.random.default_rng(5301)
    steps, gyro = [], []
    for keep in ((7,), (0, 7), (3, 4), (1, 2, 3, 4, 5, 6, 7), (1, 3, 5, 7)):
        cams, yaw, _ = scene(rng, [2] * 8, noise=1e-3)
        steps.append(emptied(cams, keep)); gyro.append(yaw + rng.normal(0, 0.02))
    return steps, gyro


def _planar_wall():
    rng = np.random.default_rng(5401)
    steps, gyro = [], []
    for counts, noise in (((3, 3), 0.0), ((3, 3), 1e-3), ((1, 0), 1e-3), ((1, 1), 1e-3), ((0, 1), 0.0)):
        cams, yaw, _ = wall_scene(rng, counts, noise)
        steps.append(cams); gyro.append(yaw + rng.normal(0, 0.02))
    return steps, gyro


def _planar_near():
    steps, gyro, lifts = [], [], []
    for d in NEAR_LIFTS:
        rng = np.random.default_rng(5402)                         # one wall, one tag lifted further and further
        cams, yaw, _ = wall_scene(rng, (3, 3), 1e-3, lift=(1, 1, d))
        steps.append(cams); gyro.append(yaw + 0.01); lifts.append(d)
    return steps, gyro, lifts


def _free_3d():
    rng = np.random.default_rng(5403)
    steps, gyro = [], []
    for noise in (0.0, 1e-3):
        cams, yaw, _ = scene(rng, (3, 3, 3), noise=noise, depths=(1.0, 2.5, 5.0))
        steps.append(cams); gyro.append(yaw + rng.normal(0, 0.02))
    return steps, gyro


def _singular_qtt():
    rng = np.random.default_rng(5404)
    steps, gyro = [], []
    for n in (1, 2):
        yaw, Rwr, twr = robot(rng)
        A, b = np.eye(3), np.array([0.1, -0.2, 0.05])            # the identity mount: u = A^T v = (0, 0, 1) exactly, M = diag(1, 1, 0)
        tags = [tag_at(rng, A, b, Rwr, twr, rng.uniform(1.0, 3.0)) for _ in range(n)]
        steps.append([(tags, np.tile([0.0, 0.0, 1.0], (4 * n, 1)), (A, b))]); gyro.append(yaw)
    return steps, gyro


def _far_and_near():
    rng = np.random.default_rng(5405)
    steps, gyro = [], []
    for noise in (0.0, 1e-4):
        cams, yaw, _ = scene(rng, (2, 2), noise=noise, depths=(0.3, 40.0), translation=2.0)
        steps.append(cams); gyro.append(yaw + rng.normal(0, 0.02))
    return steps, gyro


def _cheirality_second():
    steps, gyro = [], []
    for seed in CHEIRALITY_SECOND_SEEDS:
        cams, yaw, _ = scene(np.random.default_rng(5500 + seed), [1], noise=5e-4)
        steps.append(cams); gyro.append(yaw + np.pi)
    return steps, gyro


def impossible(seed, front=2, good=0):
    """camera 0 sees `front` tags, camera 1 the bearings of a tag that lies 1-3 m BEHIND it; `good` more tags in a camera 2"""
    rng = np.random.default_rng(seed)
    yaw, Rwr, twr = robot(rng)
    cams = []
    for c, n in enumerate((front, 1) + ((good,) if good else ())):
        A, b = mount(rng)
        tags = [tag_at(rng, A, b, Rwr, twr, rng.uniform(1.0, 3.0) * (-1.0 if c == 1 else 1.0)) for _ in range(n)]
        cams.append((tags, project(tags, A, b, Rwr, twr, rng.normal(0, 1, (n, 4, 2)) * 5e-4), (A, b)))
    return cams, yaw + rng.normal(0, 0.02)


def _cheirality_none():
    rng = np.random.default_rng(5601)
    a, ya, _ = scene(rng, (2, 1), noise=5e-4)
    b, yb, _ = scene(rng, (1, 2), noise=5e-4)
    bad, yg = impossible(5600 + CHEIRALITY_NONE_SEED)
    far, yf = impossible(5650 + CHEIRALITY_NONE_SEED, front=16)   # the points behind their camera are 64..67: beyond rig_pick's first stride
    return [a, bad, b, far], [ya, yg, yb, yf]


def _gyro_sweep(which):
    rng = np.random.default_rng(5701)
    cams, yaw, _ = scene(rng, (2, 2), noise=1e-3, yaw=0.7)
    if which == "a":
        return [cams] * len(GYRO_A), [yaw + np.radians(d) for d in GYRO_A]
    steps, gyro = [cams] * len(GYRO_B), [yaw + np.radians(d) for d in GYRO_B]
    for y, g in ((np.pi - 0.05, -np.pi + 0.1), (-np.pi + 0.05, np.pi - 0.1)):          # gyro - vision_yaw wraps across +-pi
        cams, _, _ = scene(rng, (2, 2), noise=1e-3, yaw=y)
        steps.append(cams); gyro.append(g)
    return steps, gyro


def _std_branches():
    steps, gyro = [], []
    for k, target in enumerate(STD_TARGETS):
        rng = np.random.default_rng(5801 + k)
        cams, yaw, truth = scene(rng, [4], depth=(10.0, 20.0))
        if target is not None:
            noise = [rng.normal(0, 1, (4, 4, 2))]

            def rms(c):
                tr = {}
                N.solve_rig(c, yaw, trace=tr)
                return tr["rms"]
            s = tune(lambda s: with_noise(cams, truth, noise, s), rms, target, target / 15.0)
            cams = with_noise(cams, truth, noise, s)
        steps.append(cams); gyro.append(yaw)
    return steps, gyro


def _gate_edge():
    steps, gyro, planted = [], [], []
    for k, target in enumerate((0.95, 1.05)):
        rng = np.random.default_rng(5901)
        cams, yaw, truth = scene(rng, (3, 3), depth=(1.0, 3.0))
        noise = [rng.normal(0, 1, (3, 4, 2)) * 2e-4 for _ in cams]
        noise[1][2] /= 2e-4                                       # one tag's noise is the one that is scaled: it alone sits at the gate

        def ratio(c):
            tr = {}
            NR.solve_robust(c, yaw, trace=tr)
            return tr["gate_ratio"]
        s = tune(lambda s: with_noise(cams, truth, noise, s, only=(1, 2)), ratio, target, 3e-3, power=2.0, iters=8)
        steps.append(with_noise(cams, truth, noise, s, only=(1, 2))); gyro.append(yaw)
        planted.append([0, 0] if target < 1 else None)            # (beyond the gate the restatement says what happens)
    return steps, gyro, planted


def _all_outliers():
    steps, gyro = [], []
    for seed in ALL_OUTLIERS_SEEDS:
        rng = np.random.default_rng(6000 + seed)
        cams, yaw, truth = scene(rng, (2, 2), noise=5e-4)
        cams, _ = planted_scene(rng, cams, truth, [(0, 0), (0, 1), (1, 0), (1, 1)])
        steps.append(cams); gyro.append(yaw)
    return steps, gyro


def _first_pass_not_found():
    rng = np.random.default_rng(6101)
    good, yg, _ = scene(rng, (2, 1, 6), noise=5e-4)
    bad, yb = impossible(6100 + FIRST_PASS_SEED, good=6)
    far, yf = impossible(6150 + FIRST_PASS_SEED, front=16, good=6)
    return [bad, good, far], [yb, yg, yf], [[0, 1, 0], [0, 0, 0], [0, 1, 0]]


@functools.lru_cache(maxsize=None)
def case(name):
    R = {}                                                        # the default robust parameters
    if name in ("count_one_camera", "count_one_camera_robust"):
        rb = name.endswith("robust")
        s, g, p = _count_one_camera(rb)
        return _case(name, 1, "15..64 tags in one camera: 60..256 points, the strides of 64 and 128 and their multiples", s, g,
                     R if rb else None, p if rb else None)
    if name in ("count_bit63", "count_bit63_robust"):
        rb = name.endswith("robust")
        s, g, p = _sized(5102, (64, 64), 5e-4, BIT63_PLANTED, rb)
        return _case(name, 2, "2 x 64 tags: bit 63 of a mask, global tags 63, 64 and 127", s, g, R if rb else None, p if rb else None)
    if name in ("count_full", "count_full_robust"):
        rb = name.endswith("robust")
        s, g, p = _sized(5103, (64,) * 8, 1e-3, FULL_PLANTED, rb, extra=(65,) * 8)
        return _case(name, 8, "8 x 64 = 512 tags, 2048 points: every entry of rho[] and wt[]; plain also 8 x 65", s, g, R if rb else None,
                     p if rb else None)
    if name in ("count_eight_by_five", "count_eight_by_five_robust"):
        rb = name.endswith("robust")
        a = _sized(5104, (4,) * 8, 1e-3, [(7, 3)], rb)
        b = _sized(5105, (5,) * 8, 1e-3, [(4, 4), (0, 0)], rb)
        return _case(name, 8, "8 cameras x 4 and x 5 tags: 128 and 160 points over every camera", a[0] + b[0], a[1] + b[1],
                     R if rb else None, a[2] + b[2] if rb else None)
    if name == "cams_sparse":
        s, g = _sparse()
        return _case(name, 8, "empty cameras at the front, in a row, all but the last", s, g)
    if name == "planar_wall":
        s, g = _planar_wall()
        return _case(name, 2, "coplanar scenes: a wall, one tag alone, two tags in one plane", s, g)
    if name == "planar_near":
        s, g, lifts = _planar_near()
        return _case(name, 2, "one tag off the wall by 1e-9..1e-1 m: both sides of the coplanar test", s, g, lifts=lifts)
    if name == "free_3d":
        s, g = _free_3d()
        return _case(name, 3, "tags at three depths and orientations: the free branch", s, g)
    if name == "singular_qtt":
        s, g = _singular_qtt()
        return _case(name, 1, "four (eight) bearings exactly (0, 0, 1): det(Q_tt) exactly 0", s, g, twin_only=True)
    if name == "far_and_near":
        s, g = _far_and_near()
        return _case(name, 2, "tags at 0.3 m and 40 m, mounts up to 2 m from the robot's origin", s, g)
    if name == "cheirality_second":
        s, g = _cheirality_second()
        return _case(name, 1, "gyro = true yaw + pi: a cheaper candidate is rejected for a point behind its camera", s, g)
    if name == "cheirality_none":
        s, g = _cheirality_none()
        return _case(name, 2, "every candidate rejected: no pose on a step that has tags, between two solved steps", s, g)
    if name in ("gyro_sweep_a", "gyro_sweep_b"):
        s, g = _gyro_sweep(name[-1])
        return _case(name, 2, "gyro at true yaw + 0..180 deg (a) / - 10..179 deg and across the wrap at +-pi (b)", s, g)
    if name == "std_branches":
        s, g = _std_branches()
        return _case(name, 1, "rms on both sides of 0.1, both upper clamps, both lower clamps", s, g)
    if name == "gate_edge":
        s, g, p = _gate_edge()
        return _case(name, 2, "rho_max within 0.9..1.1 of gate^2, below and above", s, g, R, p)
    if name == "all_outliers":
        s, g = _all_outliers()
        return _case(name, 2, "every tag a wrong id: every weight 0, NO_CONSENSUS", s, g, R, [None] * len(s))
    if name == "first_pass_not_found":
        s, g, p = _first_pass_not_found()
        return _case(name, 3, "no candidate in front on the first pass: the cheapest stands in, the impossible tag is dropped", s, g, R, p)
    raise KeyError(name)


NAMES = ("count_one_camera", "count_one_camera_robust", "count_bit63", "count_bit63_robust", "count_full", "count_full_robust",
         "count_eight_by_five", "count_eight_by_five_robust", "cams_sparse", "planar_wall", "planar_near", "free_3d", "singular_qtt",
         "far_and_near", "cheirality_second", "cheirality_none", "gyro_sweep_a", "gyro_sweep_b", "std_branches", "gate_edge",
         "all_outliers", "first_pass_not_found")


# ---- the restatement of a case, its stability and its conditioning ---------------------------------------------------------------------
def perturbed(cams, seed):
    """cams with every bearing component and every tag translation component multiplied by 1 +- 2^-50, the signs seeded"""
    rng = np.random.default_rng(seed)
    e = 2.0 ** -50
    out = []
    for tags, bearings, m in cams:
        b = np.asarray(bearings, float).reshape(-1, 3)
        out.append(([(R, t * (1 + e * rng.choice([-1.0, 1.0], 3))) for R, t in tags], b * (1 + e * rng.choice([-1.0, 1.0], b.shape)), m))
    return out


def _solve(c, cams, gyro):
    """(discrete results, continuous results {field: array}, the restatement's record, its read-out) of one step"""
    tr = {}
    if c["robust"] is None:
        ref = N.solve_rig(cams, gyro, trace=tr)
        fused, ftr, disc = ref, tr, ()
    else:
        ref = NR.solve_robust(cams, gyro, trace=tr, **c["robust"])
        if ref is None:
            return ("empty",), {}, None, tr
        fused, ftr = ref["fused"], tr.get("fused", {})
        disc = (ref["status"], ref["rounds"], tuple(ref["rejected"]), tr["found"], tr["alive"])
    if fused is None:
        return disc + (False,), {} if c["robust"] is None else {"worst": np.array(0.0), "best": np.array(0.0)}, ref, tr
    std = np.asarray(fused["std"], float)
    cont = {"rot": fused["rot"], "pos": fused["pos"], "yaw": np.array(fused["yaw"]), "cam_rms": np.array(fused["cam_rms"]),
            "std": np.where(std == DBL_MAX, 0.0, std), "energy": np.array(fused["energy"] / max(fused["energy"], 1e-13))}
    if c["robust"] is not None:
        cont.update(worst=np.array(ref["worst"]), best=np.array(ref["best"]))
    return disc + (True, ftr["coplanar"], ftr["winner"], ftr["std_branch"], fused["n_tags"], tuple(fused["cam_tags"])), cont, ref, tr


@functools.lru_cache(maxsize=None)
def restated(name):
    """per step: {"ref" (the restatement's record; None: no pose / an empty step), "trace", "discrete", "stable", "kappa", "bound"}"""
    c = case(name)
    out = []
    for i, (cams, gyro) in enumerate(zip(c["steps"], c["gyro"])):
        if sum(len(t) for t, _, _ in cams) == 0:
            out.append({"ref": None, "trace": {}, "discrete": ("empty",), "stable": True, "kappa": 0.0, "bound": TOL})
            continue
        disc, cont, ref, tr = _solve(c, cams, gyro)
        kappa, stable = 0.0, True
        for k in range(8):
            d2, c2, _, _ = _solve(c, perturbed(cams, [sum(map(ord, name)), i, k]), gyro)
            stable = stable and d2 == disc
            if d2 == disc:
                kappa = max([kappa] + [float(np.abs(c2[f] - cont[f]).max()) for f in cont])
        out.append({"ref": ref, "trace": tr, "discrete": disc, "stable": stable, "kappa": kappa, "bound": max(TOL, KAPPA_FACTOR * kappa)})
    return out


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def _fail(label, field, got, want, diff=None, bound=None):
    raise Mismatch(f"{label}: {field}: got {got!r}, want {want!r}" + ("" if diff is None else f", worst difference {diff:.3e} > {bound:.3e}"))


def _within(label, field, got, want, bound):
    got, want = np.asarray(got, float), np.asarray(want, float)
    diff = np.abs(np.where(got == want, 0.0, got - want))         # (DBL_MAX standard deviations are equal, not close)
    worst = float(diff.max()) if diff.size else 0.0
    if not worst <= bound:                                        # (a NaN fails)
        _fail(label, field, got.tolist(), want.tolist(), worst, bound)
    return worst


def fused_against_restatement(label, got, want, n_cams, bound):
    """a ck_rig_result_t record against np_rig's record (None: no pose): discrete fields exact, continuous ones within bound; the
    worst continuous difference"""
    if want is None:
        if got.tobytes() != bytes(got.nbytes):
            _fail(label, "record", "a pose" if got["valid"] else "non-zero bytes", "all zero")
        return 0.0
    for f, g, w in (("valid", int(got["valid"]), 1), ("n_tags", int(got["n_tags"]), want["n_tags"]),
                    ("cam_tags", list(got["cam_tags"]), list(want["cam_tags"]) + [0] * (len(got["cam_tags"]) - n_cams))):
        if g != w:
            _fail(label, f, g, w)
    worst = 0.0
    for f, w in (("rot", want["rot"]), ("pos", want["pos"]), ("yaw", want["yaw"]), ("std_devs", want["std"])):
        worst = max(worst, _within(label, f, got[f], w, bound))
    worst = max(worst, _within(label, "cam_rms", got["cam_rms"][:n_cams], want["cam_rms"], bound))
    scale = max(want["energy"], 1e-13)
    return max(worst, _within(label, "energy (relative)", got["energy"] / scale, want["energy"] / scale, bound))


def against_restatement(label, c, got, step):
    """a record of either call against the restated step"""
    want, bound = step["ref"], step["bound"]
    if c["robust"] is None:
        return fused_against_restatement(label, got, want, c["n_cams"], bound)
    if want is None:
        if got.tobytes() != bytes(got.nbytes):
            _fail(label, "record", "non-zero bytes", "all zero")
        return 0.0
    for f, g, w in (("status", int(got["status"]), want["status"]), ("rounds", int(got["rounds"]), want["rounds"]),
                    ("n_rejected", int(got["n_rejected"]), int((~want["keep"]).sum())),
                    ("rejected", [int(m) for m in got["rejected"]], list(want["rejected"]) + [0] * (len(got["rejected"]) - c["n_cams"]))):
        if g != w:
            _fail(label, f, g, w)
    worst = fused_against_restatement(label + " fused", got["fused"], want["fused"], c["n_cams"], bound)
    worst = max(worst, _within(label, "worst_inlier_rad", got["worst_inlier_rad"], want["worst"], bound))
    return max(worst, _within(label, "best_rejected_rad", got["best_rejected_rad"], want["best"], bound))


def fused_against_twin(label, got, want):
    """device against twin, as tests/test_gpu_rig.py compares them: integers equal, continuous fields within 1e-9, the energy within
    1e-9 relative + 1e-12, a record without a pose all zero"""
    for f in ("valid", "n_tags", "cam_tags"):
        if not np.array_equal(got[f], want[f]):
            _fail(label, f, got[f].tolist(), want[f].tolist())
    if not want["valid"]:
        if got.tobytes() != bytes(got.nbytes):
            _fail(label, "record", "non-zero bytes", "all zero")
        return 0.0
    worst = 0.0
    for f in ("rot", "pos", "yaw", "std_devs", "cam_rms"):
        worst = max(worst, _within(label, f, got[f], want[f], TOL))
    if not abs(got["energy"] - want["energy"]) <= 1e-9 * abs(want["energy"]) + 1e-12:
        _fail(label, "energy", float(got["energy"]), float(want["energy"]), abs(float(got["energy"] - want["energy"])), 1e-9 * abs(float(want["energy"])) + 1e-12)
    return worst


def against_twin(label, c, got, want):
    if c["robust"] is None:
        return fused_against_twin(label, got, want)
    for f in ("status", "rounds", "n_rejected", "rejected"):
        if not np.array_equal(got[f], want[f]):
            _fail(label, f, got[f].tolist(), want[f].tolist())
    worst = fused_against_twin(label + " fused", got["fused"], want["fused"])
    for f in ("worst_inlier_rad", "best_rejected_rad"):
        worst = max(worst, _within(label, f, got[f], want[f], TOL))
    return worst


def to_step(cams):
    """np_rig cameras -> what RigSolver takes"""
    from chalkydri_amd.sqpnp import iso3
    return [([iso3(t, N.mat_to_quat(R)) for R, t in tags], b, iso3(bb, N.mat_to_quat(Am))) for tags, b, (Am, bb) in cams]


def robust_params(c):
    from chalkydri_amd.rig import RobustParams
    return None if c["robust"] is None else RobustParams(**{{"gate": "gate_rad"}.get(k, k): v for k, v in c["robust"].items()})


def solve(solver, c, host=False, steps=None):
    """the case's one call on `solver` (RigSolver): solve_host or solve_batch"""
    steps = c["steps"] if steps is None else steps
    fn = solver.solve_host if host else solver.solve_batch
    return fn([to_step(s) for s in steps], c["gyro"][:len(steps)], robust=robust_params(c))


def same_but_for_the_cameras(label, got, want, idx):
    """the record of a step with empty cameras against the record of the same step with them deleted (idx: the cameras that stay):
    rot, pos, yaw, std_devs, energy and n_tags byte for byte, cam_tags and cam_rms permuted accordingly"""
    for f in ("valid", "n_tags", "rot", "pos", "yaw", "std_devs", "energy"):
        if got[f].tobytes() != want[f].tobytes():
            _fail(label, f + " (bytes)", got[f].tolist(), want[f].tolist())
    tags, rms = np.zeros_like(got["cam_tags"]), np.zeros_like(got["cam_rms"])
    tags[idx], rms[idx] = want["cam_tags"][:len(idx)], want["cam_rms"][:len(idx)]
    for f, w in (("cam_tags", tags), ("cam_rms", rms)):
        if got[f].tobytes() != w.tobytes():
            _fail(label, f + " (bytes, permuted)", got[f].tolist(), w.tolist())
