"""Draws an AprilGrid in numpy (test infrastructure, CPU only): rows x cols tags of one family with a black square in every gap
intersection — the squares touch the tags' corners, which makes every tag corner an X-saddle —, seen in perspective, blurred, with
noise, optionally with a flat grey rectangle painted over part of it.

Board coordinates are calibration.Board's: x along a row, y along a column (down, like the image), tag (r, c) on
[c pitch, c pitch + s] x [r pitch, r pitch + s] with s = tag_size and pitch = s (1 + tag_spacing); the squares lie on
[c pitch - gap, c pitch] x [r pitch - gap, r pitch] for c = 0..cols, r = 0..rows, gap = s tag_spacing.  A tag's cells are those of
np_tag_render (its [-1, 1]^2 is the tag's black square; +y is down), so detection corner k of tag t is Board.tag_corners(t)[k].
Pixel (i, j) covers [i, i + 1) x [j, j + 1); its value is the 4 x 4 supersampled area average.

Truth: uv [rows * cols][4][2], the image of every tag's four corners, and the board-to-image homography H.
"""
import numpy as np

import family_gen
import np_tag_render as R

PAPER, PATCH = 215.0, 120.0


def board_homography(rows, cols, tag_size, tag_spacing, w, h, seed, fill=0.86, tilt=15.0):
    """A pinhole view of the board: turned up to `tilt` degrees about x and y and 10 about z, placed so that the board's outline fills
    `fill` of the smaller relative frame dimension, centred.  Returns H (board metres -> pixels, H[2][2] = 1)."""
    rng = np.random.default_rng(1000 + seed)
    ax, ay, az = np.deg2rad(rng.uniform(-tilt, tilt)), np.deg2rad(rng.uniform(-tilt, tilt)), np.deg2rad(rng.uniform(-10, 10))
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    Rm = Rz @ Ry @ Rx
    pitch, gap = tag_size * (1 + tag_spacing), tag_size * tag_spacing
    x0, x1, y0, y1 = -gap, cols * pitch, -gap, rows * pitch
    centre = np.array([(x0 + x1) / 2, (y0 + y1) / 2, 0.0])
    f = 0.9 * w
    K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]])
    outline = np.array([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0.0]]) - centre

    def view(z):
        P = outline @ Rm.T + [0, 0, z]
        return P[:, :2] / P[:, 2:3] * f

    z = 1.0
    for _ in range(40):  # the distance at which the outline fills the frame as asked
        uv = view(z)
        z *= max(np.ptp(uv[:, 0]) / (fill * w), np.ptp(uv[:, 1]) / (fill * h))
    t = np.array([0, 0, z]) - Rm @ centre
    H = K @ np.column_stack([Rm[:, 0], Rm[:, 1], t])
    return H / H[2, 2]


_DRAWN = {}  # the noise-free, unblurred drawings, by view


def render(fam_p, rows=4, cols=4, tag_size=0.088, tag_spacing=0.3, first_id=0, w=643, h=481, seed=0, blur=0.0, noise=2.0, ramp=40.0,
           patch=None, ss=4, squares=True, H=None):
    """(uint8 frame [h][w], truth).  patch = (x0, y0, x1, y1) in pixels, or the four corners [4][2] of a convex quadrilateral: a flat
    grey patch painted over the scene (before the blur, like a thing lying on the board).  truth: {"uv": [rows * cols][4][2], "H": H, "hidden": [rows * cols] bool — a corner of the tag
    lies inside the patch —, "clear": [rows * cols] bool — every corner of the tag is more than 8 pixels (a window of half_win 5, its
    gradient ring and the bilinear tap) away from the patch}.  The noise-free, unblurred drawing of a view is kept and reused."""
    H = board_homography(rows, cols, tag_size, tag_spacing, w, h, seed) if H is None else np.asarray(H, float)
    key = (rows, cols, tag_size, tag_spacing, first_id, w, h, seed, ramp, ss, squares, H.tobytes())
    if key not in _DRAWN:
        _DRAWN[key] = _draw(fam_p, rows, cols, tag_size, tag_spacing, first_id, w, h, seed, ramp, ss, squares, H)
    img = _DRAWN[key].copy()
    if patch is not None:
        yy, xx = np.mgrid[0:h, 0:w] + 0.5
        img[_outside(_polygon(patch), xx, yy) <= 0] = PATCH
    if blur > 0:
        img = gaussian_blur(img, blur)
    if noise > 0:
        img = img + np.random.default_rng(7919 + seed).normal(0, noise, img.shape)
    pitch = tag_size * (1 + tag_spacing)
    uv = np.zeros((rows * cols, 4, 2))
    sq = np.array([[-1.0, 1.0], [1.0, 1.0], [1.0, -1.0], [-1.0, -1.0]]) * tag_size / 2
    for k in range(rows * cols):
        c = np.array([(k % cols) * pitch + tag_size / 2, (k // cols) * pitch + tag_size / 2]) + sq
        uv[k] = np.array(R.project(H, c[:, 0], c[:, 1])).T
    hidden, clear = np.zeros(rows * cols, bool), np.ones(rows * cols, bool)
    if patch is not None:
        d = _outside(_polygon(patch), uv[:, :, 0], uv[:, :, 1])
        hidden, clear = (d <= 0).any(1), (d > 8.0).all(1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), {"uv": uv, "H": H, "hidden": hidden, "clear": clear}


def _draw(fam_p, rows, cols, tag_size, tag_spacing, first_id, w, h, seed, ramp, ss, squares, H):
    nbits, wab, tw, rev, bx, by, codes = family_gen.tables(fam_p)
    mc = -((tw - wab) // 2)
    Hi = np.linalg.inv(H)
    yy, xx = np.mgrid[0:h, 0:w].astype(float)
    gx, gy = np.random.default_rng(seed).uniform(-1, 1, 2)
    bg = 128.0 + ramp * (gx * (xx / w - 0.5) + gy * (yy / h - 0.5))
    pitch, gap = tag_size * (1 + tag_spacing), tag_size * tag_spacing
    margin = 0.5 * gap
    off = (np.arange(ss) + 0.5) / ss
    px = np.arange(w)[None, :, None, None] + off[None, None, None, :]
    py = np.arange(h)[:, None, None, None] + off[None, None, :, None]
    px, py = np.broadcast_arrays(px, py)
    X, Y = R.project(Hi, px, py)
    on_board = (X >= -gap - margin) & (X <= cols * pitch + margin) & (Y >= -gap - margin) & (Y <= rows * pitch + margin)
    val = np.where(on_board, PAPER, np.broadcast_to(bg[:, :, None, None], px.shape))
    # position within the pitch cell: [0, s) is the tag, [s, pitch) the gap that follows it
    cxi, cyi = np.floor(X / pitch).astype(np.int64), np.floor(Y / pitch).astype(np.int64)
    lx, ly = X - cxi * pitch, Y - cyi * pitch
    in_sq = on_board & (lx >= tag_size) & (ly >= tag_size) & (cxi >= -1) & (cxi < cols) & (cyi >= -1) & (cyi < rows)
    if squares:
        val = np.where(in_sq, R.BLACK, val)
    grids = np.stack([R.tag_grid(fam_p, codes[first_id + k]) for k in range(rows * cols)])
    # a tag's cells, quiet ring included; the ring of the tag that follows reaches back into this pitch cell
    for dxc in (0, 1):
        for dyc in (0, 1):
            tcx, tcy = cxi + dxc, cyi + dyc
            u, v = (X - tcx * pitch) / tag_size * wab, (Y - tcy * pitch) / tag_size * wab
            gxi, gyi = np.floor(u).astype(np.int64) - mc, np.floor(v).astype(np.int64) - mc
            hit = on_board & (tcx >= 0) & (tcx < cols) & (tcy >= 0) & (tcy < rows) & (gxi >= 0) & (gxi < tw) & (gyi >= 0) & (gyi < tw)
            if squares:  # the squares overprint the corners of the quiet ring
                hit &= ~in_sq
            tid = np.clip(tcy, 0, rows - 1) * cols + np.clip(tcx, 0, cols - 1)
            val = np.where(hit, grids[tid, np.clip(gyi, 0, tw - 1), np.clip(gxi, 0, tw - 1)], val)
    return val.mean(axis=(2, 3))


def _polygon(patch):
    p = np.asarray(patch, float)
    if p.shape == (4,):
        x0, y0, x1, y1 = p
        p = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
    area = 0.5 * np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1])
    return p if area > 0 else p[::-1]


def _outside(poly, x, y):
    """the largest signed distance of (x, y) to the edge lines of a convex polygon: <= 0 inside; outside, a lower bound of the distance"""
    d = None
    for a, b in zip(poly, np.roll(poly, -1, axis=0)):
        e = (b - a) / np.linalg.norm(b - a)
        s = e[1] * (x - a[0]) - e[0] * (y - a[1])
        d = s if d is None else np.maximum(d, s)
    return d


def board_patch(H, x0, y0, x1, y1):
    """the image of the board rectangle [x0, x1] x [y0, y1] (metres): a patch lying on the board"""
    c = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], float)
    return np.array(R.project(H, c[:, 0], c[:, 1])).T


def gaussian_blur(img, sigma):
    r = int(np.ceil(4 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    p = np.pad(img, r, mode="edge")
    p = sum(k[i] * p[:, i:i + img.shape[1]] for i in range(2 * r + 1))
    return sum(k[i] * p[i:i + img.shape[0], :] for i in range(2 * r + 1))
