"""An AprilTag-3-STYLE tag decode in float64 (numpy), written from the published algorithm independently of oracle/detector.c
and k_decode.hip — the decode stage's reference, as np_at3_quads.py is the quad fit's.

For one quad (four corners in the detector's order) and one family it:
- computes the homography H of the quad, tag square [-1, 1]^2 to pixels, with np.linalg.solve;
- fits the white and the black gray models (least squares, a + b x + c y) to the samples just outside and just inside the
  border, and rejects the quad when the border's polarity is not the family's (reversed_border);
- samples every data bit bilinearly, subtracts the mean of the two models, sharpens the total_width grid with a Laplacian;
- reads the code word, finds the closest code by Hamming distance and reports the decision margin;
- and finds the ROTATION GEOMETRICALLY: the grid is read through H R(k 90 deg) for k = 0..3 and each word is matched against
  the codes as they are (rotation 0).  No code-word rotation function is involved, so a rotation bug that the oracle and the
  device share (code_rotate90) cannot hide here.

The pieces the detector fixes by convention are AprilTag-3's: tag (x, y) of a cell centre is 2 ((c + 0.5) / width_at_border
- 0.5); bit i is bit nbits-1-i of the word; bilinear samples are centred on pixel centres (x - 0.5); border samples read
the pixel (int(x), int(y)) and skip points outside the image; ties between candidates go to fewer quarter turns, then the
smaller id.
"""
import numpy as np

import family_gen

TAG_CORNERS = [(-1, 1), (1, 1), (1, -1), (-1, -1)]   # the detector's corner order (bottom-left, ... in the tag's frame)


def quad_homography(p):
    """H mapping (-1,-1), (1,-1), (1,1), (-1,1) to the quad's corners p[0..3]."""
    src = [(-1, -1), (1, -1), (1, 1), (-1, 1)]
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i, ((x, y), (u, v)) in enumerate(zip(src, np.asarray(p, float))):
        A[2 * i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[2 * i + 1] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[2 * i], b[2 * i + 1] = u, v
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def _proj(H, x, y):
    v = H @ np.array([x, y, 1.0])
    return v[0] / v[2], v[1] / v[2]


def _turn(k):
    """R(k * 90 deg) acting on tag coordinates."""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][k]
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def _bilinear(im, px, py):
    h, w = im.shape
    fx, fy = px - 0.5, py - 0.5
    x1, y1 = int(np.floor(fx)), int(np.floor(fy))
    x2, y2 = int(np.ceil(fx)), int(np.ceil(fy))
    if x1 < 0 or y1 < 0 or x2 >= w or y2 >= h:
        return None
    ax, ay = fx - x1, fy - y1
    return (float(im[y1, x1]) * (1 - ax) * (1 - ay) + float(im[y1, x2]) * ax * (1 - ay) + float(im[y2, x1]) * (1 - ax) * ay +
            float(im[y2, x2]) * ax * ay)


def _gray_models(im, H, wab):
    """(white, black) coefficient vectors [a, b, c] of gray = a x + b y + c, from the border samples."""
    h, w = im.shape
    rows = {True: [], False: []}
    for i in range(wab):
        t = (i + 0.5) / wab
        # (tag x01, tag y01, white?): outside (white for a normal border) and inside the border, on all four sides
        for x01, y01, white in ((-0.5 / wab, t, True), (0.5 / wab, t, False), ((wab + 0.5) / wab, t, True), ((wab - 0.5) / wab, t, False),
                                (t, -0.5 / wab, True), (t, 0.5 / wab, False), (t, (wab + 0.5) / wab, True), (t, (wab - 0.5) / wab, False)):
            tx, ty = 2 * (x01 - 0.5), 2 * (y01 - 0.5)
            px, py = _proj(H, tx, ty)
            if px < 0 or py < 0 or int(px) >= w or int(py) >= h:
                continue
            rows[white].append((tx, ty, float(im[int(py), int(px)])))
    out = []
    for white in (True, False):
        r = np.array(rows[white], float)
        X = np.stack([r[:, 0], r[:, 1], np.ones(len(r))], 1)
        out.append(np.linalg.solve(X.T @ X, X.T @ r[:, 2]))
    return out


def _read(im, H, fam, sharpening):
    """(code word, margin) read through H (rotation 0 of the family's layout), or None when the border polarity is wrong."""
    nbits, wab, tw, rev, bx, by, _ = fam
    wm, bm = _gray_models(im, H, wab)
    if (wm[2] - bm[2] < 0) != bool(rev):
        return None
    mc = -((tw - wab) // 2)
    vals = np.zeros((tw, tw))
    for i in range(nbits):
        tx, ty = 2 * ((bx[i] + 0.5) / wab - 0.5), 2 * ((by[i] + 0.5) / wab - 0.5)
        v = _bilinear(im, *_proj(H, tx, ty))
        if v is None:
            continue
        thr = (wm @ [tx, ty, 1] + bm @ [tx, ty, 1]) / 2
        vals[by[i] - mc, bx[i] - mc] = v - thr
    pad = np.pad(vals, 1)
    lap = 4 * vals - pad[:-2, 1:-1] - pad[2:, 1:-1] - pad[1:-1, :-2] - pad[1:-1, 2:]
    vals = vals + sharpening * lap
    bits = vals[by - mc, bx - mc]
    word = 0
    for v in bits:
        word = (word << 1) | int(v > 0)
    white, black = bits[bits > 0], -bits[bits <= 0]
    margin = min(white.sum() / (len(white) + 1), black.sum() / (len(black) + 1))
    return word, margin


def decode(im, quad, fam_p, sharpening=0.25, max_hamming=3):
    """Decode one quad (4x2 corners) as family fam_p.  Returns None or a dict id, hamming, rotation, margin, c, p."""
    fam = family_gen.tables(fam_p)
    codes = fam[6]
    H = quad_homography(quad)
    best = None
    for k in range(4):
        Hk = H @ _turn(k)
        r = _read(im, Hk, fam, sharpening)
        if r is None:
            return None            # the polarity test does not depend on k (the border samples are the same points)
        word, margin = r
        d = family_gen.popcount(codes ^ np.uint64(word))
        i = int(np.argmin(d))      # the first (smallest) id at the smallest distance
        if best is None or d[i] < best[0]:
            best = (int(d[i]), k, i, margin, Hk)
    hd, k, i, margin, Hk = best
    if hd > max_hamming:
        return None
    return {"id": i, "hamming": hd, "rotation": k, "margin": margin,
            "c": np.array(_proj(Hk, 0.0, 0.0)), "p": np.array([_proj(Hk, x, y) for x, y in TAG_CORNERS])}
