"""The coloured-piece detector restated in numpy / scipy from DESIGN.md §4r — from the definition, not from the C: HSV with its
divisions, scipy's morphology and labelling, the filter, the order and the derived doubles.  What the host twin is checked against."""
import numpy as np
from scipy import ndimage

HAS_BEARING, HAS_GROUND, AT_BORDER = 1, 2, 4
TRUNCATED, OVERFLOW = 1, 2
S8 = np.ones((3, 3), bool)


def ycc_rgb(ycc):
    """libjpeg's ycc_rgb_convert of uint8 [..., 3] (Y, Cb, Cr) triples, clamped."""
    y, cb, cr = (ycc[..., i].astype(np.int64) for i in range(3))
    r = y + ((91881 * (cr - 128) + 32768) >> 16)
    g = y + ((-22554 * (cb - 128) - 46802 * (cr - 128) + 32768) >> 16)
    b = y + ((116130 * (cb - 128) + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def rgb_hsv(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    v = np.maximum(np.maximum(r, g), b)
    m = np.minimum(np.minimum(r, g), b)
    d = v - m
    s = np.where(v == 0, 0, (255 * d) // np.maximum(v, 1))
    hn_r = 30 * (g - b) + np.where(g < b, 180 * d, 0)
    hn_g = 30 * (b - r) + 60 * d
    hn_b = 30 * (r - g) + 120 * d
    hn = np.where(v == r, hn_r, np.where(v == g, hn_g, hn_b))   # ties: R, then G, then B
    h = np.where(d == 0, 0, ((2 * hn + d) // np.maximum(2 * d, 1)) % 180)
    return np.stack([h, s, v], -1).astype(np.uint8)


def class_mask(cls, rgb):
    """bool [H][W]: the pixels class `cls` (any object with the ColorClass fields) holds."""
    hsv = rgb_hsv(rgb).astype(np.int64)
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    if cls.h_min > cls.h_max:
        hue = (h >= cls.h_min) | (h <= cls.h_max)
    else:
        hue = (h >= cls.h_min) & (h <= cls.h_max)
    return hue & (s >= cls.s_min) & (s <= cls.s_max) & (v >= cls.v_min) & (v <= cls.v_max)


def morph(mask, erode, dilate):
    if erode:
        mask = ndimage.binary_erosion(mask, structure=S8, iterations=erode, border_value=0)
    if dilate:
        mask = ndimage.binary_dilation(mask, structure=S8, iterations=dilate, border_value=0)
    return mask


def pack(mask):
    """bool [..., W] -> uint32 [..., ceil(W/32)]: bit x & 31 of word x >> 5."""
    W = mask.shape[-1]
    ww = (W + 31) // 32
    padded = np.zeros(mask.shape[:-1] + (ww * 32,), np.uint8)
    padded[..., :W] = mask
    return np.packbits(padded, axis=-1, bitorder="little").view("<u4")


def unproject(model, k, u, v):
    """OPENCV5 (model 0: the reference's fixed-point undistortion) or EUCM / UCM (1, 2): unit bearing, ok."""
    mx, my = (u - k[2]) / k[0], (v - k[3]) / k[1]
    if model == 0:
        k1, k2, p1, p2, k3 = k[4:9]
        x, y, ok = mx, my, False
        for _ in range(50):
            r2 = x * x + y * y
            rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
            nx = (mx - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / rad
            ny = (my - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / rad
            done = (nx - x) ** 2 + (ny - y) ** 2 < 1e-24
            x, y = nx, ny
            if done:
                ok = True
                break
        b = np.array([x, y, 1.0])
        return b / np.linalg.norm(b), ok
    alpha, beta = k[4], (1.0 if model == 2 else k[5])
    r2 = mx * mx + my * my
    if alpha > 0.5 and not r2 < 1.0 / (beta * (2 * alpha - 1)):
        return np.zeros(3), False
    kz = (1 - alpha * alpha * beta * r2) / (alpha * np.sqrt(1 - (2 * alpha - 1) * beta * r2) + 1 - alpha)
    b = np.array([mx, my, kz])
    return b / np.linalg.norm(b), True


def quat_mat(q):
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def ground_point(camera, mount, ground_z, max_range, u, v):
    """(x, y) of the robot frame where the ray of pixel (u, v) meets z = ground_z, or None.  camera: (model, k); mount: (t, q), cam from robot."""
    b, ok = unproject(camera[0], camera[1], u, v)
    if not ok:
        return None
    R, t = quat_mat(mount[1]), np.asarray(mount[0], float)
    o, d = -R.T @ t, R.T @ b
    if not d[2] < 0 or not o[2] > ground_z:
        return None
    s = (ground_z - o[2]) / d[2]
    if not s <= max_range:
        return None
    return (o + s * d)[:2]


def components(mask):
    """Per 8-connected component: dict of area, box, seed and sums, in label order."""
    H, W = mask.shape
    lab, n = ndimage.label(mask, structure=S8)
    ys, xs = np.nonzero(mask)
    ids = lab[ys, xs]
    out = []
    for i in range(1, n + 1):
        sel = ids == i
        x, y = xs[sel].astype(np.int64), ys[sel].astype(np.int64)
        out.append(dict(area=int(x.size), x0=int(x.min()), y0=int(y.min()), x1=int(x.max()), y1=int(y.max()),
                        seed=int((y * W + x).min()), sx=int(x.sum()), sy=int(y.sum()), sxx=int((x * x).sum()),
                        sxy=int((x * y).sum()), syy=int((y * y).sum())))
    return out


def passes(cls, c):
    bw, bh, N = c["x1"] - c["x0"] + 1, c["y1"] - c["y0"] + 1, c["area"]
    if N < cls.min_area or (cls.max_area and N > cls.max_area):
        return False
    if 1000 * N < cls.min_fill_permille * bw * bh:
        return False
    if cls.min_aspect_permille * bh > 1000 * bw:
        return False
    return not (cls.max_aspect_permille and 1000 * bw > cls.max_aspect_permille * bh)


def derived(c, W, H, camera=None, mount=None, ground_z=0.0, max_range=20.0):
    """The record's doubles and flags from a component's integers."""
    N = float(c["area"])
    mx, my = c["sx"] / N, c["sy"] / N
    cov = np.array([[c["sxx"] / N - mx * mx, c["sxy"] / N - mx * my], [c["sxy"] / N - mx * my, c["syy"] / N - my * my]])
    a, b, cc = cov[0, 0], cov[0, 1], cov[1, 1]
    rt = np.hypot(a - cc, 2 * b)
    l1, l2 = max((a + cc + rt) / 2, 0.0), max((a + cc - rt) / 2, 0.0)
    if rt > 0:
        ax = np.array([(a - cc + rt) / 2, b]) if a >= cc else np.array([b, (rt - (a - cc)) / 2])
        ax = ax / np.linalg.norm(ax)
        if ax[0] < 0 or (ax[0] == 0 and ax[1] < 0):
            ax = -ax
    else:
        ax = np.array([1.0, 0.0])
    flags = AT_BORDER if (c["x0"] == 0 or c["y0"] == 0 or c["x1"] == W - 1 or c["y1"] == H - 1) else 0
    bearing, ground = np.zeros(3), np.zeros(2)
    if camera is not None:
        bb, ok = unproject(camera[0], camera[1], mx + 0.5, my + 0.5)
        if ok:
            bearing, flags = bb, flags | HAS_BEARING
        if mount is not None:
            gp = ground_point(camera, mount, ground_z, max_range, (c["x0"] + c["x1"] + 1) / 2.0, c["y1"] + 1.0)
            if gp is not None:
                ground, flags = gp, flags | HAS_GROUND
    return dict(cx=mx + 0.5, cy=my + 0.5, major=np.sqrt(l1), minor=np.sqrt(l2), axis=ax, bearing=bearing, ground=ground, flags=flags)


def detect(classes, rgb, erode=0, dilate=0, max_targets=16, max_components=4096, cap=None, camera=None, mount=None, max_range=20.0):
    """One frame rgb [H][W][3] -> (per class the list of written records as dicts, counts, status)."""
    H, W, _ = rgb.shape
    cap = max_targets if cap is None else cap
    recs, counts, status = [], [], 0
    for ci, cls in enumerate(classes):
        comps = [c for c in components(morph(class_mask(cls, rgb), erode, dilate)) if c["area"] >= cls.min_area]
        if len(comps) > max_components:
            status |= OVERFLOW
            recs.append([]); counts.append(0)
            continue
        good = sorted([c for c in comps if passes(cls, c)], key=lambda c: (-c["area"], c["seed"]))
        nw = min(len(good), max_targets, cap)
        if nw < len(good):
            status |= TRUNCATED
        counts.append(len(good))
        recs.append([dict(c, class_id=ci, **derived(c, W, H, camera, mount, cls.ground_z, max_range)) for c in good[:nw]])
    return recs, counts, status
