"""Draws tags of any ck_family_t in numpy (test infrastructure, CPU only), independently of the library's renderer (synth.c).

A tag is its family's total_width x total_width cell grid in tag coordinates, where [-1, 1]^2 is the outer edge of the border
(the square the detector's quads fit) and cell (x, y) of the family's bit tables spans
[2 x / wab - 1, 2 (x + 1) / wab - 1] x [2 y / wab - 1, 2 (y + 1) / wab - 1].  Colours: a data cell shows its code bit (1 white,
0 black), the border ring is black (white when reversed_border), every other cell has the colour opposite to the border.
Pixel (i, j) covers [i, i + 1) x [j, j + 1) of the image plane; its value is the supersampled area average of the tag (through
the inverse of the tag's homography) over a background with a linear ramp, plus Gaussian noise.

Ground truth: corners H(-1, 1), H(1, 1), H(1, -1), H(-1, -1) and centre H(0, 0) for a tag drawn at its codes' rotation 0, the
order the detector reports corners in.
"""
import numpy as np

import family_gen

BLACK, WHITE = 35.0, 215.0


def homography(corners):
    """H with H(-1,-1) = corners[0], H(1,-1) = corners[1], H(1,1) = corners[2], H(-1,1) = corners[3] (H[2][2] = 1)."""
    src = [(-1, -1), (1, -1), (1, 1), (-1, 1)]
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i, ((x, y), (u, v)) in enumerate(zip(src, np.asarray(corners, float))):
        A[2 * i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[2 * i + 1] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[2 * i], b[2 * i + 1] = u, v
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def project(H, x, y):
    x, y = np.asarray(x, float), np.asarray(y, float)
    z = H[2, 0] * x + H[2, 1] * y + H[2, 2]
    return (H[0, 0] * x + H[0, 1] * y + H[0, 2]) / z, (H[1, 0] * x + H[1, 1] * y + H[1, 2]) / z


def tag_grid(fam_p, code, flip=()):
    """Grey level of every cell of the total_width grid, [y - min_coord][x - min_coord]; `flip`: bit indices drawn inverted."""
    nbits, wab, tw, rev, bx, by, _ = family_gen.tables(fam_p)
    mc = -((tw - wab) // 2)
    border, other = (WHITE, BLACK) if rev else (BLACK, WHITE)
    g = np.full((tw, tw), other)
    for y in range(tw):
        for x in range(tw):
            cx, cy = x + mc, y + mc
            if 0 <= cx < wab and 0 <= cy < wab and (cx in (0, wab - 1) or cy in (0, wab - 1)):
                g[y, x] = border
    code = int(code)
    for i in range(nbits):
        bit = ((code >> (nbits - 1 - i)) & 1) ^ (1 if i in flip else 0)
        g[by[i] - mc, bx[i] - mc] = WHITE if bit else BLACK
    return g


def pose(cx, cy, side, angle_deg, tilt=(0.0, 0.0)):
    """Corners (detector order of the tag square's corners (-1,-1), (1,-1), (1,1), (-1,1)) of a square of `side` pixels centred
    at (cx, cy), turned by angle_deg, with a mild perspective given by tilt = (tx, ty) (fractions of the side)."""
    a = np.deg2rad(angle_deg)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    sq = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], float)
    pts = sq * (1 + np.outer(sq[:, 0] * tilt[0] + sq[:, 1] * tilt[1], [1, 1]))
    return (pts * side / 2) @ R.T + [cx, cy]


def scene(fams, seed, w=643, h=481, cols=3, rows=2, side=(60, 110), noise=1.5, flips=0):
    """A frame of cols x rows tags, one per cell of a grid over the image, each of a family drawn from `fams` (pointers), a random
    id, turned by a quarter turn (every one of them in any four consecutive cells) plus up to 20 degrees, mildly tilted.  Tags never overlap and stay inside the frame.
    flips: number of data bits drawn inverted in every tag.  Truth entries gain `family` (index into fams) and `id`."""
    rng = np.random.default_rng(seed)
    tags, meta = [], []
    cw, ch = w / cols, h / rows
    for r in range(rows):
        for c in range(cols):
            fi = int(rng.integers(0, len(fams)))
            nbits, wab, tw, _, _, _, codes = family_gen.tables(fams[fi])
            i = int(rng.integers(0, len(codes)))
            ext = tw / wab * 1.15                          # the grid's extent in units of the border's side, tilt and turn included
            s = min(rng.uniform(*side), 0.95 * min(cw, ch) / ext / 1.42)
            ang = 90.0 * ((r * cols + c + seed) % 4) + rng.uniform(-20, 20)
            tilt = tuple(rng.uniform(-0.03, 0.03, 2))
            flip = tuple(int(b) for b in rng.choice(nbits, flips, replace=False)) if flips else ()
            tags.append({"fam": fams[fi], "code": int(codes[i]), "corners": pose((c + 0.5) * cw, (r + 0.5) * ch, s, ang, tilt), "flip": flip})
            meta.append((fi, i))
    img, truth = render(w, h, tags, seed=seed, noise=noise)
    for t, (fi, i) in zip(truth, meta):
        t["family"], t["id"] = fi, i
    return img, truth


def render(w, h, tags, seed=0, noise=2.0, ramp=40.0, ss=4):
    """tags: list of dicts with fam (POINTER(Family)), code (int), corners (4x2, see pose) and optional flip (bit indices).
    Returns (uint8 frame [h][w], truth list of {fam_index, code, corners, center})."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(float)
    gx, gy = rng.uniform(-1, 1, 2)
    img = 128.0 + ramp * (gx * (xx / w - 0.5) + gy * (yy / h - 0.5))
    truth = []
    off = (np.arange(ss) + 0.5) / ss
    for t in tags:
        nbits, wab, tw, rev, bx, by, _ = family_gen.tables(t["fam"])
        mc = -((tw - wab) // 2)
        H = homography(t["corners"])
        Hi = np.linalg.inv(H)
        grid = tag_grid(t["fam"], t["code"], t.get("flip", ()))
        # pixel box of the whole grid (the quiet ring included)
        e0, e1 = 2.0 * mc / wab - 1, 2.0 * (mc + tw) / wab - 1
        ex, ey = project(H, [e0, e1, e1, e0], [e0, e0, e1, e1])
        x0, x1 = max(int(np.floor(ex.min())) - 1, 0), min(int(np.ceil(ex.max())) + 1, w)
        y0, y1 = max(int(np.floor(ey.min())) - 1, 0), min(int(np.ceil(ey.max())) + 1, h)
        c = np.array(project(H, [-1, 1, 1, -1], [1, 1, -1, -1])).T
        truth.append({"fam": t["fam"], "code": int(t["code"]), "corners": c, "center": np.array(project(H, 0.0, 0.0))})
        if x0 >= x1 or y0 >= y1:
            continue
        px = (np.arange(x0, x1)[None, :, None, None] + off[None, None, None, :])
        py = (np.arange(y0, y1)[:, None, None, None] + off[None, None, :, None])
        px, py = np.broadcast_arrays(px, py)
        tx, ty = project(Hi, px, py)
        cx = np.floor((tx + 1) * wab / 2).astype(np.int64) - mc     # grid column of the sample
        cy = np.floor((ty + 1) * wab / 2).astype(np.int64) - mc
        inside = (cx >= 0) & (cx < tw) & (cy >= 0) & (cy < tw)
        bg = np.broadcast_to(img[y0:y1, x0:x1, None, None], px.shape)
        val = np.where(inside, grid[np.clip(cy, 0, tw - 1), np.clip(cx, 0, tw - 1)], bg)
        img[y0:y1, x0:x1] = val.mean(axis=(2, 3))
    img = img + rng.normal(0, noise, img.shape) if noise > 0 else img
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), truth
