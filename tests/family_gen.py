"""Test tag families: ck_family_t tables of the geometries AprilTag-3's other families have (odd bit counts, data bits outside
the border, reversed borders, code words up to 64 bits, grids up to total_width 16), with stand-in codebooks.

The bit layout follows AprilTag-3's convention, which the built-in tag36h11 and tag16h5 tables have: one quarter's cells,
then the same cells turned 1, 2 and 3 times about the grid centre, and for an odd bit count the centre cell last.  That is
what makes code_rotate90 a 90 degree turn of the tag.  The codebooks are greedy random lexicodes from a fixed seed: a code is
kept when it is at least `min_hamming` bits from all four rotations of every kept code and from its own three other rotations.
They are NOT upstream's codes; only the geometry matches the family named in MATRIX.

CPU only: numpy and ctypes.
"""
import ctypes as C

import numpy as np

from chalkydri_amd import _abi as A


def ring(lo, hi):
    """Cells on the outline of the square [lo, hi] x [lo, hi]."""
    return [(x, y) for y in range(lo, hi + 1) for x in range(lo, hi + 1) if x in (lo, hi) or y in (lo, hi)]


def square(lo, hi):
    return [(x, y) for y in range(lo, hi + 1) for x in range(lo, hi + 1)]


def turn(cell, wab):
    """One quarter turn about the grid centre ((wab - 1) / 2, (wab - 1) / 2): the turn that maps the cell of bit i to the cell
    of bit i + nbits // 4 in AprilTag-3's layouts."""
    x, y = cell
    return (wab - 1 - y, x)


def layout(cells, wab):
    """bit_x, bit_y for a rotation-symmetric set of cells: quarter, its three turns, then the centre cell if present."""
    cells = set(cells)
    c2 = wab - 1                                         # twice the centre coordinate
    centre = (c2 // 2, c2 // 2) if c2 % 2 == 0 else None
    rest = cells - {centre}
    # the fundamental domain of the quarter turn, in doubled coordinates about the centre: u > 0, v >= 0
    quarter = sorted((c for c in rest if 2 * c[0] - c2 > 0 and 2 * c[1] - c2 >= 0),
                     key=lambda c: (max(abs(2 * c[0] - c2), abs(2 * c[1] - c2)), c[1], c[0]))
    order = []
    for k in range(4):
        for c in quarter:
            for _ in range(k):
                c = turn(c, wab)
            order.append(c)
    assert set(order) == rest and len(order) == len(rest), "cell set is not symmetric under a quarter turn"
    if centre in cells:
        order.append(centre)
    return [c[0] for c in order], [c[1] for c in order]


def popcount(a):
    return np.bitwise_count(np.asarray(a, np.uint64)).astype(np.int64)


def rotate90(codes, nbits):
    """AprilTag-3's rotate90 on an array of code words (with the 64-bit mask done right)."""
    codes = np.asarray(codes, np.uint64)
    p, l = nbits, 0
    if nbits % 4 == 1:
        p, l = nbits - 1, 1
    u = np.uint64
    w = ((codes >> u(l)) << u(p // 4 + l)) | ((codes >> u(3 * p // 4 + l)) << u(l)) | (codes & u(l))
    mask = (1 << nbits) - 1
    return w & u(mask)


def lexicode(nbits, min_hamming, ncodes, seed):
    """Greedy random lexicode under rotation.  Returns a uint64 array of up to `ncodes` codes."""
    rng = np.random.default_rng(seed)
    kept_rots = np.zeros(0, np.uint64)                   # every kept code in its four orientations
    kept = []
    tries = 0
    while len(kept) < ncodes and tries < 200000:
        tries += 1
        c = np.uint64(int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4)))
        c = c & np.uint64((1 << nbits) - 1)
        rots = [c]
        for _ in range(3):
            rots.append(rotate90(np.array([rots[-1]]), nbits)[0])
        if min(int(popcount(c ^ r)) for r in rots[1:]) < min_hamming:
            continue
        if len(kept_rots) and int(popcount(kept_rots ^ c).min()) < min_hamming:
            continue
        kept.append(c)
        kept_rots = np.concatenate([kept_rots, np.array(rots, np.uint64)])
    return np.array(kept, np.uint64)


# name -> (nbits, width_at_border, total_width, reversed_border, data cells, min_hamming, ncodes)
MATRIX = {
    # like tagStandard41h12: inner 3x3 (centre bit last) and the outermost ring, outside the border
    "std41r": (41, 5, 9, 1, square(1, 3) + ring(-2, 6), 10, 120),
    "std41n": (41, 5, 9, 0, square(1, 3) + ring(-2, 6), 10, 120),
    # like tagCircle21h7: inner 3x3 and the middle three cells of each side of the outermost ring
    "circ21r": (21, 5, 9, 1, square(1, 3) + [c for c in ring(-2, 6) if 1 <= c[0] <= 3 or 1 <= c[1] <= 3], 6, 40),
    # like tagStandard52h13: inner 4x4 and the outermost ring
    "std52r": (52, 6, 10, 1, square(1, 4) + ring(-2, 7), 12, 120),
    # 64-bit words: an 8x8 data area like tag36h11's 6x6, and a 16-cell grid with two data rings
    "full64": (64, 10, 12, 0, square(1, 8), 14, 150),
    "full64w": (64, 14, 16, 0, ring(1, 12) + ring(4, 9), 14, 60),
}

_keep = {}    # families of MATRIX already built, by (name, seed)
_alive = []   # ctypes buffers of every table handed out (ck_family_t holds raw pointers into them)


def make(name, seed=None):
    """POINTER(A.Family) for a family of MATRIX, built once per process."""
    key = (name, seed)
    if key in _keep:
        return _keep[key]
    nbits, wab, tw, rev, cells, mh, nc = MATRIX[name]
    bx, by = layout(cells, wab)
    assert len(bx) == nbits
    codes = lexicode(nbits, mh, nc, seed if seed is not None else 1000 + sum(map(ord, name)))
    _keep[key] = family_from(name, nbits, wab, tw, rev, bx, by, codes, mh)
    return _keep[key]


def family_from(name, nbits, wab, tw, rev, bx, by, codes, min_hamming, n_upstream=None):
    """A ck_family_t over caller-owned tables (kept alive in this module)."""
    n = len(codes)
    ccodes = (C.c_uint64 * max(n, 1))(*[int(c) for c in codes])
    cbx = (C.c_uint32 * max(len(bx), 1))(*[v & 0xFFFFFFFF for v in bx])
    cby = (C.c_uint32 * max(len(by), 1))(*[v & 0xFFFFFFFF for v in by])
    fam = A.Family()
    fam.name = name.encode()[:31]
    fam.nbits, fam.ncodes = nbits, n
    fam.codes = C.cast(ccodes, C.POINTER(C.c_uint64))
    fam.bit_x = C.cast(cbx, C.POINTER(C.c_uint32))
    fam.bit_y = C.cast(cby, C.POINTER(C.c_uint32))
    fam.width_at_border, fam.total_width, fam.reversed_border = wab, tw, rev
    fam.min_hamming = min_hamming
    fam.n_upstream = n if n_upstream is None else n_upstream
    p = C.pointer(fam)
    _alive.append((p, ccodes, cbx, cby, fam))
    return p


def tables(fam_p):
    """(nbits, wab, tw, reversed, bit_x int array, bit_y int array, codes uint64 array) of a ck_family_t pointer."""
    f = fam_p.contents
    bx = np.array([C.c_int32(f.bit_x[i]).value for i in range(f.nbits)], np.int64)
    by = np.array([C.c_int32(f.bit_y[i]).value for i in range(f.nbits)], np.int64)
    codes = np.array([f.codes[i] for i in range(f.ncodes)], np.uint64)
    return f.nbits, f.width_at_border, f.total_width, f.reversed_border, bx, by, codes


def cell_grid(fam_p, code):
    """total_width x total_width grid of the code's bits (-1 where no data bit sits), indexed [y - min_coord][x - min_coord]."""
    nbits, wab, tw, _, bx, by, _ = tables(fam_p)
    mc = -((tw - wab) // 2)
    g = np.full((tw, tw), -1, np.int64)
    code = int(code)
    for i in range(nbits):
        g[by[i] - mc, bx[i] - mc] = (code >> (nbits - 1 - i)) & 1
    return g
