"""Frames for the row-table tests of k_emit2's count pass (tests/test_gpu_emit_rows.py on the device, tests/test_emit_row_host.py for
the proof that the frames reach what they are for).  Nothing here touches the GPU.

The count pass (chalkydri_amd/csrc/k_clusters.hip, ck_emit_row.h) turns the six staged words around a pixel row — (x-1..x+1, y) and
(x-1..x+1, y+1) — into one word of predicate bits and reads the row's leaders from a table.  `rows` restates, in numpy and from the
oracle's labels, what a row is: how many leaders (distinct partner components among its points), whether it absorbs the twin of
its right neighbour, whether it drops its own (-1,1) point; `places` says where a row sits among the places the kernel treats
differently: inside a 64 x 16 emit tile, on a tile seam (the thread's staged words come from the neighbouring tile's pixels), and
in the first / last emitting column and row."""
import numpy as np

import cluster_cases as cc

DARK, LIGHT = 40, 220
SIZES = ((66, 17), (67, 18), (129, 33), (130, 35))   # a seam in x and in y, ragged last columns and rows, widths no multiple of 4
MIN_COMPONENT = (5, 25)
SKIP = np.int64(-1)


def _grid(w, h):
    return np.mgrid[0:h, 0:w]


def _bw(mask):
    return np.where(mask, LIGHT, DARK).astype(np.uint8)


def stairs(w, h, down, shift=0):
    """a diagonal boundary in steps of 2 x 2 pixels: every step has a straight piece each way, so a twin at every step"""
    yy, xx = _grid(w, h)
    xs = xx if down else (w - 1 - xx)
    return _bw((yy + shift) // 2 > (xs // 2) % ((h + 1) // 2 + 1))


def stripes(w, h, s, vertical, shift=0):
    yy, xx = _grid(w, h)
    return _bw((((xx if vertical else yy) + shift) // s) & 1 == 1)


def checker(w, h, cell, shift=0):
    yy, xx = _grid(w, h)
    return _bw((((xx + shift) // cell + (yy + shift) // cell) & 1) == 1)


def blobs(w, h, density, seed):
    """random 2 x 2 cells, light with probability `density`"""
    rng = np.random.default_rng(seed)
    cells = rng.random(((h + 1) // 2, (w + 1) // 2)) < density
    return _bw(np.kron(cells, np.ones((2, 2), bool))[:h, :w])


def lattice(w, h, px, py, ox, oy):
    """one dark component, a lattice of one-pixel lines px / py apart, around light cells: at every crossing the dark component meets
    four different light ones inside one pixel's neighbourhood"""
    yy, xx = _grid(w, h)
    return _bw(~(((xx + ox) % px == 0) | ((yy + oy) % py == 0)))


def frames(w, h):
    """name -> frame, for one size"""
    f = {}
    for down in (True, False):
        for shift in (0, 1):
            f[f"stairs {'down' if down else 'up'} +{shift}"] = stairs(w, h, down, shift)
    for s in (1, 2, 3):
        for vertical in (False, True):
            for shift in ((0, 1) if s > 1 else (0,)):
                f[f"stripes {s} {'v' if vertical else 'h'} +{shift}"] = stripes(w, h, s, vertical, shift)
    for cell in (3, 5):
        for shift in (0, 1, 2):
            f[f"checker {cell} +{shift}"] = checker(w, h, cell, shift)
    for i, density in enumerate((0.25, 0.5, 0.75)):
        f[f"blobs {density}"] = blobs(w, h, density, 100 * w + 10 * h + i)
    f["lattice 21 x 8"] = lattice(w, h, 21, 8, 0, 1)      # crossings at x = 63 and y = 15: on the seams
    f["lattice 16 x 7"] = lattice(w, h, 16, 7, 15, 6)     # crossings at x = 1 and y = 1: first emitting column and row
    f["lattice from the far rim"] = lattice(w, h, 16, 7, 16 - (w - 2) % 16, 7 - (h - 2) % 7)   # ... at x = w - 2 and y = h - 2
    return f


def rim_noise():
    """(w, h, min_component_px, name -> frame): noise at min_component_px = 1.  Pixels that touch — side by side or one above the
    other — and have one colour are one component, so of a row's four partners (x-1..x+1, y+1) and (x+1, y) at most two can be
    different components of the other colour: a row has at most two leaders.  The one exception is the frame's last column, whose
    pixels the segmentation joins to nothing: each is a component of one pixel, alive only at min_component_px = 1, and column
    w - 2 then has rows of three leaders.  Four do not occur in any frame (B0, B1, B2 would have to be three components): that
    entry of the table is reached by tests/cpp/emit_row_check.cpp alone."""
    return 130, 35, 1, {f"noise {seed}": cc.frame("noise", 130, 35, seed) for seed in range(3)}


# ---- what a row is, from the oracle's labels ---------------------------------------------------------------------------------------
def staged(th, lab, sz, min_component_px):
    """the staged word of every pixel: its component (and colour), or SKIP"""
    word = lab.astype(np.int64) | ((th == 255).astype(np.int64) << 40)
    return np.where((th == 127) | (sz.astype(np.int64) < min_component_px), SKIP, word)


def rows(th, lab, sz, min_component_px, twins=True):
    """per emitting pixel (arrays [h-2][w-2], pixel (x, y) at [y-1][x-1]): leaders, absorb, drop, and the two geometric conditions
    without their gate on the neighbour's column (would_absorb, would_drop)"""
    h, w = th.shape
    S = staged(th, lab, sz, min_component_px)
    white = (th == 255)
    c = lambda dx, dy: S[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    wc = lambda dx, dy: white[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    A0, A1, A2, B0, B1, B2 = c(-1, 0), c(0, 0), c(1, 0), c(-1, 1), c(0, 1), c(1, 1)
    P = [A2, B1, B0, B2]
    PW = [wc(1, 0), wc(0, 1), wc(-1, 1), wc(1, 1)]
    ok = [(A1 != SKIP) & (p != SKIP) & (pw != wc(0, 0)) for p, pw in zip(P, PW)]
    xs = np.arange(1, w - 1)[None, :]
    would_absorb = ok[3] & (((A1 == A2) & (B2 == B1)) | ((A1 == B1) & (B2 == A2)))
    would_drop = ok[2] & (((A1 == A0) & (B0 == B1)) | ((A1 == B1) & (B0 == A0)))
    absorb = would_absorb & (xs + 1 <= w - 2) & twins
    drop = would_drop & (xs - 1 >= 1) & twins
    ok[2] = ok[2] & ~drop
    leaders = np.zeros(A1.shape, np.int64)
    for k in range(4):
        first = ok[k].copy()
        for j in range(k):
            first &= ~(ok[j] & (P[j] == P[k]))
        leaders += first
    return dict(leaders=leaders, absorb=absorb, drop=drop, would_absorb=would_absorb, would_drop=would_drop)


def places(w, h):
    """name -> mask [h-2][w-2] over the emitting pixels"""
    ys, xs = np.mgrid[1:h - 1, 1:w - 1]
    rim = (xs == 1) | (xs == w - 2) | (ys == 1) | (ys == h - 2)
    seam = ((xs % cc.ETW == cc.ETW - 1) & (xs + 1 <= w - 1)) | ((xs % cc.ETW == 0) & (xs > 0)) | ((ys % cc.ETH == cc.ETH - 1) & (ys + 1 <= h - 1))
    return {"interior": ~rim & ~seam, "seam": seam & ~rim, "first column": xs == 1, "last column": xs == w - 2, "first row": ys == 1,
            "last row": ys == h - 2}


KINDS = ("0 leaders", "1 leader", "2 leaders", "absorb", "drop", "absorb and drop")


def kinds(r):
    return {"0 leaders": r["leaders"] == 0, "1 leader": r["leaders"] == 1, "2 leaders": r["leaders"] == 2, "absorb": r["absorb"], "drop": r["drop"],
            "absorb and drop": r["absorb"] & r["drop"]}
