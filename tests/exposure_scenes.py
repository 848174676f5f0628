"""Radiance scenes of the exposure meter's closed-loop tests (test infrastructure, CPU only).

A scene is a radiance image in [0, 1]: a mid-grey panel with low-contrast tags (tests/np_tag_render.py) beside a strip of
multi-octave texture whose radiance spans a decade and a half, as a view with a window and a shadow does.  The camera of the
tests photographs it as clip(255 radiance E) (np_exposure.photograph).  The tags' contrast is low enough that an exposure 8x
under the best one leaves less than min_white_black_diff between their cells; the strip keeps some gradient alive at either
extreme, which is what any gradient-based meter needs in order to move."""
import math

import numpy as np

import np_exposure as N
import np_tag_render as R

W, H, PANEL = 640, 360, 480
BASE, CONTRAST = 0.3, 0.05
# measured with the numpy restatement: steps to settle from 8x under / over, and the band |ln(E / E*)| it stays in
STEPS, BAND = 10, 0.92


def texture(seed, h, w, lo=0.02, hi=0.6, octaves=5):
    """exp of a sum of bilinearly interpolated random grids: smooth at every scale, log-radiance spread over [lo, hi]."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((h, w))
    for o in range(octaves):
        cells = 2 ** (o + 1)
        g = rng.uniform(-1, 1, (cells + 2, cells + 2))
        y, x = np.linspace(0, cells, h, endpoint=False), np.linspace(0, cells, w, endpoint=False)
        y0, x0 = y.astype(int), x.astype(int)
        fy, fx = (y - y0)[:, None], (x - x0)[None, :]
        a = g[y0][:, x0] * (1 - fy) * (1 - fx) + g[y0 + 1][:, x0] * fy * (1 - fx) + g[y0][:, x0 + 1] * (1 - fy) * fx + g[y0 + 1][:, x0 + 1] * fy * fx
        acc += a / (1.5 ** o)
    acc = (acc - acc.min()) / (acc.max() - acc.min())
    return np.exp(math.log(lo) + acc * (math.log(hi) - math.log(lo)))


def radiance(seed):
    """(radiance [H][W] in [0, 1], truth of the tags: np_tag_render.render's, with `id`)."""
    import family_gen
    from chalkydri_amd import _lib
    fam = _lib.family("tag36h11")
    codes = family_gen.tables(fam)[6]
    rng = np.random.default_rng(seed)
    tags, ids = [], []
    for r in range(2):
        for c in range(3):
            i = int(rng.integers(0, 30))
            tags.append({"fam": fam, "code": int(codes[i]),
                         "corners": R.pose((c + 0.5) * PANEL / 3, (r + 0.5) * H / 2, rng.uniform(60, 80), rng.uniform(-20, 20))})
            ids.append(i)
    img, truth = R.render(PANEL, H, tags, seed=seed, noise=0.0, ramp=0.0)
    for t, i in zip(truth, ids):
        t["id"] = i
    rad = np.empty((H, W))
    rad[:, :PANEL] = BASE + CONTRAST * (img.astype(float) / 255.0 - 0.5)
    rad[:, PANEL:] = texture(seed, H, W - PANEL)
    return rad, truth


def best_exposure(rad, lo=0.02, hi=60.0, n=161):
    """E*: the exposure at which the gradient information of the plain image (gamma = 1) is largest, by brute force."""
    P, lut = N.Params(), N.luts()
    k1 = P.gamma.index(1.0)
    es = np.exp(np.linspace(math.log(lo), math.log(hi), n))
    m = [N.metric(P, N.stats(N.photograph(rad, e), lut))[k1] for e in es]
    return float(es[int(np.argmax(m))])
