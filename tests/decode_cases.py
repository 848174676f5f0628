"""Inputs and CPU-side bookkeeping of the parity tests of the decode stage (tests/test_gpu_decode.py on the device,
tests/test_decode_cases_host.py for the proof that the cases reach what they name).  Nothing here touches the GPU.

The decode stage (chalkydri_amd/csrc/k_decode.hip: k_decode, k_finalize) solves a quad's homography, fits two gray models to the
border samples, reads the family's bits, sharpens, searches the codebook for the nearest code under four rotations, and leaves a
candidate; k_finalize sorts a frame's candidates and drops duplicates.  A case is a dict: frames [n][h][w], quads (one list of
ck_quad_t per frame: the drawn corners, or deliberate variations), settings, truth (per frame: the drawn (id, corners) by quad
index, where one exists) and cap.  measure(name) checks with the case's cond_* function, on the oracle's readout
(pyoracle.decode_trace), that the case reaches the edge it is named for and returns the figures it measured.  The expected detections always come from the oracle.

Everything is drawn by tests/np_tag_render.py over families of tests/family_gen.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from chalkydri_amd import _abi as A  # noqa: E402

SINGULAR, BORDER_SENSE, SIGN, HAMMING, MARGIN, CANDIDATE, NONFINITE = range(7)   # pyoracle.DECODE_EXITS
PASS = 768                                                            # codes one pass of k_decode's search covers (64 lanes x DEC_CPL 12)
DET_CAP = 256                                                         # the handle's detections per frame
M36 = (1 << 36) - 1


# ---- families --------------------------------------------------------------------------------------------------------------------------
_fams = {}


def _grown(base, nbits, n, seed, skip=()):
    """base codes, then distinct random nbits-bit words up to n codes"""
    rng = np.random.default_rng(seed)
    codes, seen = [int(c) for c in base[:n]], {int(c) for c in base} | set(skip)
    while len(codes) < n:
        c = (int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4))) & ((1 << nbits) - 1)
        if c not in seen:
            seen.add(c)
            codes.append(c)
    return codes


TIE_WORD_FLIPS = ((3, 20), (9, 30))   # bits of the tie word by which the (rotation 1, small id) and the (rotation 0, large id) code differ from it


def tie_word():
    """The word drawn in ties_rot: a fixed random word, far from every other code of t36rot (the readout shows two pairs at distance 2)."""
    return 0x5A3C96E1B


def fam(name):
    """POINTER(ck_family_t) by name: a built-in one, one of family_gen.MATRIX, or
    t36n<k> / f64n<k>: tag36h11's / full64's layout and codes, grown to k codes with distinct random words;
    t36sym: code 0 and the all-ones code (ids 0, 1), then built-in codes;  t36dup: 900 codes, id 800 a copy of id 3;
    t36rot: 900 codes, id 2 and id 700 equidistant from tie_word() under rotation 1 and rotation 0."""
    import family_gen as fg
    from chalkydri_amd import family
    if name in _fams:
        return _fams[name]
    if name.startswith("tag"):
        p = family(name)
    elif name in fg.MATRIX:
        p = fg.make(name)
    else:
        base = fg.make("full64") if name.startswith("f64") else family("tag36h11")
        nbits, wab, tw, rev, bx, by, codes = fg.tables(base)
        seed = 7000 + sum(map(ord, name))
        if name[3] == "n":
            cs = _grown(codes, nbits, int(name[4:]), seed)
        elif name == "t36sym":
            cs = [0, M36] + [int(c) for c in codes[:30]]
        elif name == "t36dup":
            cs = _grown(codes, nbits, 900, seed)
            cs[800] = cs[3]
        elif name == "t36rot":
            w = tie_word()
            cs = _grown(codes, nbits, 900, seed, skip=(w,))
            cs[2] = int(fg.rotate90(np.array([w], np.uint64), 36)[0]) ^ (1 << TIE_WORD_FLIPS[0][0]) ^ (1 << TIE_WORD_FLIPS[0][1])
            cs[700] = w ^ (1 << TIE_WORD_FLIPS[1][0]) ^ (1 << TIE_WORD_FLIPS[1][1])
        else:
            raise KeyError(name)
        p = fg.family_from(name, nbits, wab, tw, rev, list(bx), list(by), cs, 0)
    _fams[name] = p
    return p


def _families(settings):
    return tuple(fam(n) for n in settings.get("families", ("tag36h11",)))


def _cfg_kw(settings):
    return {k: v for k, v in settings.items() if k not in ("families", "quad_sigma")}


def config(w, h, settings):
    from chalkydri_amd import default_config
    return default_config(w, h, families=_families(settings), **_cfg_kw(settings))


def detector(w, h, n, settings):
    from chalkydri_amd.detector import AprilTagDetector
    kw = _cfg_kw(settings)
    return AprilTagDetector(w, h, max_batch=n, families=_families(settings), quad_sigma=settings.get("quad_sigma", 0.0),
                            bits_corrected=kw.pop("max_hamming", 3), **kw)


# ---- quads and drawing ---------------------------------------------------------------------------------------------------------------
def quad(corners, reversed_border=0):
    """ck_quad_t with p[0..3] = the images of the tag square's (-1,-1), (1,-1), (1,1), (-1,1): a tag drawn with these corners reads at rotation 0"""
    q = A.Quad()
    for i in range(4):
        q.p[i][0], q.p[i][1] = float(corners[i][0]), float(corners[i][1])
    q.reversed_border = int(reversed_border)
    q.rep0, q.rep1 = 0, 1
    return q


def box(x0, y0, side):
    return np.array([(x0, y0), (x0 + side, y0), (x0 + side, y0 + side), (x0, y0 + side)], float)


def cycled(corners, k):
    return np.roll(np.asarray(corners, float), -k, axis=0)


def draw(w, h, tags, seed=1, noise=1.0):
    """tags: (family name, id or ("word", w), corners, flip bits) -> frame"""
    import family_gen as fg
    import np_tag_render as tr
    items = []
    for name, ident, corners, flip in tags:
        p = fam(name)
        code = ident[1] if isinstance(ident, tuple) else int(fg.tables(p)[6][ident])
        items.append({"fam": p, "code": code, "corners": np.asarray(corners, float), "flip": tuple(flip)})
    return tr.render(w, h, items, seed=seed, noise=noise)[0]


def truth_corners(corners):
    """the corners a detection of a tag drawn with `corners` reports at rotation 0: H(-1,1), H(1,1), H(1,-1), H(-1,-1)"""
    c = np.asarray(corners, float)
    return c[[3, 2, 1, 0]]


def _case(frames, quads, settings, truth=None, cap=DET_CAP, max_batch=None):
    frames = np.ascontiguousarray(frames, np.uint8)
    return {"frames": frames, "quads": quads, "settings": settings, "truth": truth or [{} for _ in quads], "cap": cap,
            "max_batch": max_batch or len(frames)}


def _sheet(w, h, name, ids, side, pitch, seed, flips=0, x0=4, y0=4):
    """tags of `ids` on a grid of `pitch` pixels, axis-aligned at integer positions: (frame, quads, truth)"""
    rng = np.random.default_rng(seed)
    nbits = fam(name).contents.nbits
    cols = (w - x0) // pitch
    tags, quads, truth = [], [], {}
    for k, i in enumerate(ids):
        c = box(x0 + (k % cols) * pitch, y0 + (k // cols) * pitch, side)
        assert c[2][1] <= h, "sheet too small"
        flip = tuple(int(b) for b in rng.choice(nbits, flips, replace=False)) if flips else ()
        tags.append((name, i, c, flip))
        quads.append(quad(c, fam(name).contents.reversed_border))
        truth[k] = (i, truth_corners(c))
    return draw(w, h, tags, seed=seed), quads, truth


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
SEARCH = [("t36n%d" % k, 40, 52) for k in (767, 768, 769, 1537, 2115)] + [("f64n%d" % k, 50, 64) for k in (767, 768, 769, 1537, 2115)]


def search_ids(ncodes):
    """in the first pass, the last id of every pass, the first of the next, the very last"""
    ids = {5, ncodes - 1}
    for k in range(PASS, ncodes + 1, PASS):
        ids |= {k - 1} | ({k} if k < ncodes else set())
    return sorted(i for i in ids if i < ncodes)


def case_search(name, side, pitch):
    ids = search_ids(fam(name).contents.ncodes)
    f, q, t = _sheet(280, 200, name, ids, side, pitch, seed=len(name) + side)
    return _case([f], [q], {"families": [name]}, [t])


def case_ties(which):
    if which == "sym":      # all-black and all-white words: four rotations tie, the margin is exactly 0
        f, q, t = _sheet(160, 80, "t36sym", [0, 1, 5], 40, 52, seed=3, )
        return _case([f], [q], {"families": ["t36sym"]}, [t])
    if which == "dup":      # one code at ids 3 and 800 (another pass): the smaller id
        f, q, t = _sheet(160, 80, "t36dup", [3, 801], 40, 52, seed=4)
        return _case([f], [q], {"families": ["t36dup"]}, [t])
    c = box(20, 20, 40)     # (rotation 0, id 700) against (rotation 1, id 2), both two bits away
    f = draw(160, 80, [("t36rot", ("word", tie_word()), c, ())], seed=5)
    return _case([f], [[quad(c)]], {"families": ["t36rot"]}, [{0: (700, truth_corners(c))}])


def case_hamming(mh):
    """flips of exactly max_hamming and max_hamming + 1 bits"""
    name, tags, quads, truth = "tag36h11", [], [], {}
    rng = np.random.default_rng(20 + mh)
    for k, (i, nflip) in enumerate([(7, mh), (8, mh + 1), (100, mh), (586, mh + 1)]):
        c = box(10 + 52 * k, 12, 40)
        tags.append((name, i, c, tuple(int(b) for b in rng.choice(36, nflip, replace=False))))
        quads.append(quad(c))
        if nflip <= mh:
            truth[k] = (i, truth_corners(c))
    return _case([draw(232, 64, tags, seed=6 + mh)], [quads], {"families": [name], "max_hamming": mh}, [truth])


SHARPEN_FAMS = (("std41n", 9), ("std52r", 10), ("full64w", 16))     # total_width 9, 10 and 16 (the whole 256-entry grid)


def case_sharpen(sharpening):
    tags, quads, truth = [], [], {}
    x = 24
    for k, (name, tw) in enumerate(SHARPEN_FAMS):
        p = fam(name).contents
        side = 6 * p.width_at_border
        c = box(x + 6 * (tw - p.width_at_border) // 2, 30, side)
        x += 6 * tw + 24
        tags.append((name, 3 + k, c, (1, 7)))
        quads.append(quad(c, p.reversed_border))
        truth[k] = (3 + k, truth_corners(c))
    return _case([draw(x, 160, tags, seed=9)], [quads], {"families": [n for n, _ in SHARPEN_FAMS], "decode_sharpening": sharpening}, [truth])


OVER_W, OVER_H = 420, 400
OVERHANG = {"even": ([0, 2, 4, 6, 8, 10, 12], [0, 2, 4, 6, 8, 10, 12]), "odd": ([1, 3, 5, 7, 7.4, 9, 11, 13], [1, 3, 5, 7, 9, 11, 13])}


def case_overhang(which):
    """40-pixel tag36h11 tags (5 pixels per cell, integer positions: bit centres on pixel centres) hanging over the four sides of the
    frame by the listed pixels: left and right sides down the frame, top and bottom across it"""
    w, h = OVER_W, OVER_H
    lr, tb = OVERHANG[which]
    tags, quads, truth = [], [], {}
    def put(c, k):
        i = (0, 5, 17)[k % 3]
        tags.append(("tag36h11", i, c, ()))
        truth[len(quads)] = (i, truth_corners(c))
        quads.append(quad(c))
    for k, o in enumerate(lr):
        put(box(-o, 8 + 48 * k, 40), k)
        put(box(w - 40 + o, 8 + 48 * k, 40), k + 1)
    for k, o in enumerate(tb):
        put(box(50 + 46 * k, -o, 40), k + 2)
        put(box(50 + 46 * k, h - 40 + o, 40), k)
    return _case([draw(w, h, tags, seed=11, noise=0.5)], [quads], {"families": ["tag36h11"]}, [truth])


MODEL_W = 96


def case_model():
    """quads on a 96 x 96 frame whose gray models cannot be solved, with every bit sample inside the frame: [0] the whole frame (every
    white sample outside, every black one inside), [1] the frame is the data area (every black sample outside; the white ones lie
    further out, so they are outside too: a convex frame that holds every white sample holds the black ones; model_strip has the
    frame between them), [2] only the six middle samples of the left white and black columns inside (one side: both 3 x 3 systems
    are singular), [3] the whole frame again with a reversed border under std41r: NaN < 0 is false, which a normal border passes
    and a reversed one does not, so this one leaves through the sign test.  t36sym holds the all-zero word, so the search does not
    reject first what the NaN thresholds read as an all-black word."""
    w = MODEL_W
    rng = np.random.default_rng(12)
    f = rng.integers(30, 220, (w, w)).astype(np.uint8)
    qs = [quad(box(0, 0, w)), quad(box(-16, -16, 128)), quad([(6, -16), (102, -16), (102, 112), (6, 112)]), quad(box(0, 0, w), 1)]
    return _case([f], [qs], {"families": ["t36sym", "std41r"]})


def case_model_strip():
    """A 96 x 16 frame that lies between the samples of a sheared quad of 40-pixel cells (cell (u, v) at x = 30 + 40 u, y = -122 + 40 v +
    20 u): one white sample of the left column (10, 8) and one bit (90, 8) are inside, every black sample is outside — the frame's
    edge falls between the white column and the black one.  The black model is NaN, nothing comes back."""
    rng = np.random.default_rng(24)
    f = rng.integers(30, 220, (16, 96)).astype(np.uint8)
    return _case([f], [[quad([(30, -122), (350, 38), (350, 358), (30, 198)])]], {"families": ["t36sym"]})


ZZ_QUADS = [[(16, 16), (32, 16), (48, 16), (16, 48)], [(8, 8), (8, 40), (8, 72), (40, 8)]]   # zz == 0 at two border samples each


def random_grid_quads(seed, n, lo=0, hi=64, step=4):
    rng = np.random.default_rng(seed)
    return rng.integers(lo // step, hi // step + 1, (n, 4, 2)) * float(step)


def degenerate_frame():
    f, _, _ = _sheet(80, 80, "tag36h11", [9], 40, 52, seed=13, x0=20, y0=20)
    return f


def case_degenerate(oracle=None):
    """[0..2] four equal corners, four collinear corners, a bow-tie; [3, 4] two coincident corners, three collinear corners; [5, 6]
    ZZ_QUADS; then the first hits with a non-finite sample among 4000 random quads with corners on a 4-pixel grid (seed 14)."""
    import pyoracle
    f = degenerate_frame()
    qs = [[(30, 30)] * 4, [(10, 10), (20, 20), (40, 40), (70, 70)], [(20, 20), (60, 60), (60, 20), (20, 60)],
          [(20, 20), (60, 20), (60, 20), (20, 60)], [(20, 20), (40, 20), (60, 20), (40, 60)]] + ZZ_QUADS
    cand = random_grid_quads(14, 4000)
    settings = {"families": ["tag36h11"]}
    _, _, recs, _, _ = pyoracle.decode_trace(f, config(80, 80, settings), [quad(c) for c in cand])
    hits = [cand[i] for i in np.flatnonzero(recs["n_wild"] > 0)[:12]]
    return _case([f], [[quad(c) for c in qs + hits]], settings)


FIN_W, FIN_H, FIN_PITCH = 420, 400, 20
FIN_COUNTS = (255, 256, 257, 300)


def case_finalize_counts():
    """255, 256, 257 and 300 distinct 16-pixel tags, one frame each: more candidates than k_finalize has threads, and det_cap"""
    frames, quads, truth = [], [], []
    for n in FIN_COUNTS:
        f, q, t = _sheet(FIN_W, FIN_H, "tag36h11", list(range(n)), 16, FIN_PITCH, seed=15, x0=2, y0=2)
        frames.append(f); quads.append(q); truth.append(t)
    return _case(frames, quads, {"families": ["tag36h11"]}, truth)


def case_finalize_dups():
    """frame 0: one tag, its quad twice and cycled by 1, 2, 3; id 9 twice far apart; id 12 with a second quad 2 px off; id 20 twice,
    the centre of one on the LINE of the other's edge, outside the quad (power-of-two coordinates): a cross product is exactly zero,
    but it does not decide (the other three edges already say outside; finalize_edge has the zero that decides).
    frame 1: ids 38, 39, 40 around n_upstream = 39."""
    a, far1, far2, ov = box(16, 16, 40), box(80, 16, 40), box(200, 100, 40), box(144, 16, 40)
    z1, z2 = box(64, 96, 32), box(128, 112, 32)           # z1's centre (80, 112) lies on the line of z2's top edge y = 112
    tags = [("tag36h11", 4, a, ()), ("tag36h11", 9, far1, (2,)), ("tag36h11", 9, far2, ()), ("tag36h11", 12, ov, ()),
            ("tag36h11", 20, z1, ()), ("tag36h11", 20, z2, ())]
    q0 = [quad(a), quad(a), quad(cycled(a, 1)), quad(cycled(a, 2)), quad(cycled(a, 3)), quad(far1), quad(far2), quad(ov), quad(ov + 2.0),
          quad(z1), quad(z2)]
    f1, q1, t1 = _sheet(256, 160, "tag36h11", [38, 39, 40], 40, 52, seed=17)
    return _case([draw(256, 160, tags, seed=16), f1], [q0, q1], {"families": ["tag36h11"]}, [{0: (4, truth_corners(a))}, t1])


EDGE_A, EDGE_B = (64, 96, 32), (80, 96, 32)


def case_finalize_edge():
    """Two quads of 32 pixels over one black rectangle on a bright frame, both read as t36sym's all-black id 0 with margin 0.0: the centre
    of each, (80, 112) and (96, 112), lies exactly ON an edge of the other (x = 80, x = 96), inside its span.  The zero cross product
    decides: counted as neither sign the point is inside and the second is a duplicate; counted with the other sign both are kept."""
    f = np.full((160, 192), 215, np.uint8)
    f[96:128, 64:112] = 35
    return _case([f], [[quad(box(*EDGE_A)), quad(box(*EDGE_B))]], {"families": ["t36sym"]})


def case_finalize_nan():
    """Quads whose candidates have a corner that is not finite (zz == 0 at a tag corner), each TWICE and once with its corners cycled, under
    tag16h5 at max_hamming 3, which reads a code out of almost anything: ZZ_QUADS and hits of a seeded search among 4000 random
    integer-corner quads, kept when the readout shows them decode (exit NONFINITE).  Equal candidates with a NaN corner are what
    det_cmp cannot order; both sides leave no candidate for them."""
    import pyoracle
    f = degenerate_frame()
    settings = {"families": ["tag16h5"], "max_hamming": 3}
    cand = [np.array(q, float) for q in ZZ_QUADS] + [cycled(q, k) for q in ZZ_QUADS for k in (1, 2, 3)] + list(random_grid_quads(31, 4000))
    _, _, recs, _, _ = pyoracle.decode_trace(f, config(80, 80, settings), [quad(c) for c in cand])
    hits = [cand[i] for i in np.flatnonzero(recs["exit"] == NONFINITE)[:6]]
    qs = []
    for c in hits:
        qs += [quad(c), quad(c), quad(cycled(c, 1))]
    good, qg, _ = _sheet(80, 80, "tag16h5", [3], 36, 40, seed=25, x0=22, y0=22)     # and one tag that decodes, on a frame of its own
    return _case([f, good], [qs, qg + qg], settings)


def case_finalize_two_families():
    """two families of one border sense with the same first 587 codes: every quad leaves two candidates; the caller's cap is below the count"""
    f, q, t = _sheet(256, 120, "tag36h11", [1, 2, 3, 40, 41, 42], 40, 52, seed=18)
    return _case([f], [q], {"families": ["tag36h11", "t36n767"]}, [t], cap=5)


def case_posed():
    """tags turned by any angle and tilted, at fractional positions, normal and reversed border: corners no float holds exactly, so the
    order of the elimination's steps (the pivot among the four rows whose first entry is +-1) shows in the last bits of H"""
    import np_tag_render as tr
    rng = np.random.default_rng(23)
    tags, quads, truth = [], [], {}
    for k in range(6):
        name = ("tag36h11", "std41r")[k % 2]
        side = 44.0 + 3.7 * k
        c = tr.pose(60.3 + 100.1 * (k % 3), 62.7 + 112.9 * (k // 3), side, 17.0 + 61.3 * k, tuple(rng.uniform(-0.05, 0.05, 2)))
        tags.append((name, 10 + k, c, ()))
        quads.append(quad(c, fam(name).contents.reversed_border))
        truth[k] = (10 + k, truth_corners(c))
    return _case([draw(320, 240, tags, seed=23)], [quads], {"families": ["tag36h11", "std41r"]}, [truth])


BATCH_QUAD_CAP = 32


def case_batch(which):
    """frames with 0, 1 and quad_cap (32) quads side by side on a handle of 6 frames; 'dec2': quad_decimate 2; 'sigma': quad_sigma 0.8 at
    decimation 1 (decode reads the filtered frame: the test takes it from the device)"""
    w, h = 180, 120
    full, qf, tf = _sheet(w, h, "tag36h11", list(range(50, 50 + BATCH_QUAD_CAP)), 16, 20, seed=19, x0=4, y0=4)
    one, q1, t1 = _sheet(w, h, "tag36h11", [77], 40, 52, seed=20)
    empty = draw(w, h, [], seed=21)
    settings = {"families": ["tag36h11"], "max_quads_per_frame": BATCH_QUAD_CAP}
    if which == "dec2":
        settings["quad_decimate"] = 2
    if which == "sigma":
        settings["quad_sigma"] = 0.8
    return _case([empty, one, full], [[], q1, qf], settings, [{}, t1, tf], max_batch=6)


CASES = {}
for _n, _s, _p in SEARCH:
    CASES["search_" + _n] = (case_search, (_n, _s, _p))
for _k in ("sym", "dup", "rot"):
    CASES["ties_" + _k] = (case_ties, (_k,))
for _k in (0, 3):
    CASES["hamming_%d" % _k] = (case_hamming, (_k,))
for _k, _v in (("0", 0.0), ("025", 0.25), ("1", 1.0)):
    CASES["sharpen_" + _k] = (case_sharpen, (_v,))
for _k in OVERHANG:
    CASES["overhang_" + _k] = (case_overhang, (_k,))
CASES["posed"] = (case_posed, ())
CASES["model"] = (case_model, ())
CASES["model_strip"] = (case_model_strip, ())
CASES["degenerate"] = (case_degenerate, ())
CASES["finalize_counts"] = (case_finalize_counts, ())
CASES["finalize_dups"] = (case_finalize_dups, ())
CASES["finalize_edge"] = (case_finalize_edge, ())
CASES["finalize_nan"] = (case_finalize_nan, ())
CASES["finalize_two_families"] = (case_finalize_two_families, ())
for _k in ("plain", "dec2", "sigma"):
    CASES["batch_" + _k] = (case_batch, (_k,))
NAMES = list(CASES)
_built = {}


def case(name):
    if name not in _built:
        fn, args = CASES[name]
        _built[name] = fn(*args)
    return _built[name]


# ---- the oracle's view ---------------------------------------------------------------------------------------------------------------
def expected(oracle, c, images=None):
    """Per frame (ck_detection_t bytes, count, status) as ck_decode_quads_batch has to return them, and the readouts: the oracle with the
    handle's 256 detections per frame, then the caller's cap.  images: what decode reads when that is not the frame (quad_sigma)."""
    frames = c["frames"] if images is None else images
    n, h, w = frames.shape
    cfg = config(w, h, c["settings"])
    out, reads = [], []
    for i in range(n):
        dets, raw, recs, call, ov = oracle.decode_trace(frames[i], cfg, c["quads"][i], cap=DET_CAP)
        st = A.CK_FRAME_DETS_OVERFLOW if ov else 0
        if any(d["id"] >= cfg.families[d["family"]].contents.n_upstream for d in dets):
            st |= A.CK_FRAME_UNVERIFIED_ID
        cnt = len(dets)
        if cnt > c["cap"]:
            cnt, st = c["cap"], st | A.CK_FRAME_DETS_OVERFLOW
        out.append((raw[:cnt * 96], cnt, st))
        reads.append((dets, recs, call))
    return out, reads


def check_truth(c, reads):
    """every detection that belongs to a drawn tag has its id, and corners within a pixel of the drawn ones"""
    for i, (dets, recs, _) in enumerate(reads):
        for k, (ident, corners) in c["truth"][i].items():
            r = recs[recs["quad"] == k]
            for rr in r[r["exit"] == CANDIDATE]:
                if rr["best_hd"] == 0 and rr["n_best"] == 1:
                    assert rr["id"] == ident and rr["rot"] == 0, (i, k, rr)
        for d in dets:
            near = [(ident, cs) for ident, cs in c["truth"][i].values() if np.abs(cs - d["p"]).max() < 1.0]
            if near and d["hamming"] == 0:
                assert any(ident == d["id"] or d["family"] > 0 for ident, _ in near), (i, d)


def run_case(det_factory, oracle, name, shuffle=None):
    """The case (a name, or a case dict) through AprilTagDetector.decode_quads: a list of what differs from the oracle (empty: equal), and the bytes returned.
    shuffle: a seed; the quad lists are permuted (the result may not depend on it)."""
    c = name if isinstance(name, dict) else case(name)
    name = "case" if isinstance(name, dict) else name
    frames = c["frames"]
    n, h, w = frames.shape
    quads = c["quads"]
    if shuffle is not None:
        rng = np.random.default_rng(shuffle)
        quads = [[q[j] for j in rng.permutation(len(q))] for q in quads]
    det = det_factory(w, h, c["max_batch"], c["settings"])
    try:
        images = det.quad_image(frames) if c["settings"].get("quad_sigma") else None
        got, status = det.decode_quads(quads, frames, cap=c["cap"], return_status=True, raw=True)
        det.upload(frames)
        again, status2 = det.decode_quads(quads, None, cap=c["cap"], return_status=True, raw=True)   # on the staged frames
    finally:
        det.close()
    want, reads = expected(oracle, c, images)
    check_truth(c, reads)
    bad = []
    for i in range(n):
        if (got[i], len(got[i]) // 96, status[i]) != want[i]:
            bad.append((name, i, "count %d status %d, oracle count %d status %d" % (len(got[i]) // 96, status[i], want[i][1], want[i][2])))
        if again[i] != got[i] or status2[i] != status[i]:
            bad.append((name, i, "the staged frames give other bytes"))
    return bad, b"".join(got) + bytes(status), sum(cnt for _, cnt, _ in want)


# ---- conditions: what the oracle's readout has to show -------------------------------------------------------------------------------
def _all(reads):
    recs = np.concatenate([r for _, r, _ in reads])
    call = {k: sum(c[k] for _, _, c in reads) for k in reads[0][2]}
    return recs, call


def cond_search(c, reads, name):
    recs, _ = _all(reads)
    ids = search_ids(fam(name).contents.ncodes)
    assert list(recs["id"]) == ids and (recs["exit"] == CANDIDATE).all() and (recs["best_hd"] == 0).all() and (recs["n_best"] == 1).all()
    ncodes = fam(name).contents.ncodes
    assert (ncodes > PASS) == any(i >= PASS for i in ids) and ncodes - 1 in ids
    return {"ncodes": ncodes, "ids": ids}


def cond_ties(c, reads, which):
    recs, _ = _all(reads)
    if which == "sym":
        assert list(recs["n_best"][:2]) == [4, 4] and list(recs["rot"][:2]) == [0, 0] and list(recs["id"][:2]) == [0, 1]
        assert list(recs["margin"][:2]) == [0.0, 0.0] and (recs["exit"] == CANDIDATE).all()
        return {"n_best": [4, 4], "margin": [0.0, 0.0]}
    if which == "dup":
        assert recs["n_best"][0] == 2 and recs["id"][0] == 3 and recs["best_hd"][0] == 0 and recs["exit"][0] == CANDIDATE and recs["id"][1] == 801
        return {"n_best": 2, "id": 3}
    r = recs[0]
    assert r["code"] == tie_word() and r["n_best"] == 2 and r["best_hd"] == 2 and (r["rot"], r["id"]) == (0, 700) and r["exit"] == CANDIDATE
    return {"n_best": 2, "best_hd": 2, "chosen": (0, 700), "other": (1, 2)}


def cond_hamming(c, reads, mh):
    recs, _ = _all(reads)
    assert list(recs["best_hd"]) == [mh, mh + 1, mh, mh + 1] and list(recs["exit"]) == [CANDIDATE, HAMMING, CANDIDATE, HAMMING]
    return {"best_hd": [mh, mh + 1] * 2}


def cond_sharpen(c, reads, sharpening):
    recs, _ = _all(reads)
    own = recs[recs["quad"] == recs["family"]]
    assert (own["exit"] == CANDIDATE).all() and list(own["id"]) == [3, 4, 5] and (own["best_hd"] == 2).all()
    return {"margins": [round(float(m), 3) for m in own["margin"]]}


def cond_overhang(c, reads, which):
    recs, _ = _all(reads)
    e = int(np.bitwise_or.reduce(recs["edges"]))
    want = (2 | 8) if which == "even" else (1 | 4 | 8 | 16 | 32)
    assert e & want == want, (e, want)
    assert (recs["bits_outside"] > 0).any() and ((recs["exit"] == CANDIDATE) & (recs["n_white"] + recs["n_black"] < 64)).any()
    assert (recs["exit"] != CANDIDATE).any()
    return {"edges": e, "decoded": int((recs["exit"] == CANDIDATE).sum()), "of": len(recs),
            "decoded_with_bits_outside": int(((recs["exit"] == CANDIDATE) & (recs["bits_outside"] > 0)).sum())}


def cond_posed(c, reads):
    recs, call = _all(reads)
    own = recs[recs["family"] == recs["quad"] % 2]
    assert call["candidates"] == 6 and (own["exit"] == CANDIDATE).all() and list(own["id"]) == list(range(10, 16))
    assert list(own["best_hd"]) == [0, 0, 0, 0, 0, 2] and own["bits_outside"][5] == 3   # (the last tag's outer data ring leaves the frame)
    assert (recs[recs["family"] != recs["quad"] % 2]["exit"] == BORDER_SENSE).all()
    p = np.array([[q.p[i][j] for i in range(4) for j in range(2)] for q in c["quads"][0]])
    assert (p != np.round(p * 1024) / 1024).all()
    return {"candidates": 6}


def cond_model(c, reads):
    recs, call = _all(reads)
    assert call["candidates"] == 0
    rev = recs[(recs["quad"] == 3) & (recs["family"] == 1)][0]      # the reversed border: out through the sign test on a NaN model
    assert rev["exit"] == SIGN and rev["model_nan"] & 1 and rev["n_white"] == 0 and rev["n_black"] > 0
    assert (recs[(recs["quad"] < 3) & (recs["family"] == 1)]["exit"] == BORDER_SENSE).all()
    recs = recs[(recs["quad"] < 3) & (recs["family"] == 0)]
    assert (recs["n_white"][0], recs["n_black"][0]) == (0, 32) and (recs["n_white"][1], recs["n_black"][1]) == (0, 0)
    assert (recs["n_white"][2], recs["n_black"][2]) == (6, 6) and (recs["bits_outside"] == 0).all()
    assert (recs["model_nan"] != 0).all() and all(r["exit"] in (SIGN, MARGIN) for r in recs)
    assert all(r["exit"] != MARGIN or np.isnan(r["margin"]) for r in recs) and (recs["exit"] == MARGIN).any()
    return {"exits": [int(x) for x in recs["exit"]], "model_nan": [int(x) for x in recs["model_nan"]]}


def cond_model_strip(c, reads):
    recs, call = _all(reads)
    r = recs[0]
    assert call["candidates"] == 0 and (r["n_white"], r["n_black"]) == (1, 0) and r["bits_outside"] == 35 and r["model_nan"] & 2
    assert r["exit"] == MARGIN and np.isnan(r["margin"])
    return {"n_white": 1, "n_black": 0, "bits_inside": 1, "exit": int(r["exit"])}


def cross_products(p, x, y):
    """point_in_quad's four cross products of the point (x, y) against the detection corners p"""
    return [(p[(i + 1) % 4][0] - p[i][0]) * (y - p[i][1]) - (p[(i + 1) % 4][1] - p[i][1]) * (x - p[i][0]) for i in range(4)]


def cond_finalize_edge(c, reads):
    import pyoracle
    dets, recs, call = reads[0]
    assert (recs["exit"] == CANDIDATE).all() and list(recs["id"]) == [0, 0] and list(recs["margin"]) == [0.0, 0.0]
    assert call["candidates"] == 2 and call["duplicates"] == 1 and len(dets) == 1 and call["zero_cross"] >= 1 and call["equal_pairs"] == 1
    f = c["frames"][0]
    cfg = config(f.shape[1], f.shape[0], c["settings"])
    a, b = (pyoracle.decode_quads(f, cfg, [q])[0] for q in c["quads"][0])     # each quad's detection on its own
    decisive = 0
    for k, d in ((a, b), (b, a)):
        cr = cross_products(k["p"], d["c"][0], d["c"][1])
        assert sorted(np.sign(cr)) in ([-1, -1, -1, 0], [0, 1, 1, 1]), cr      # one zero, the three others of one sign
        decisive += 1
    return {"zero_cross": call["zero_cross"], "decisive_zeros": decisive}


def cond_finalize_nan(c, reads):
    (d0, r0, c0), (d1, r1, c1) = reads
    same = r0[np.arange(len(r0)) % 3 < 2]                  # each quad and its repetition; the cycled copy may read with finite corners
    assert len(same) >= 12 and (same["exit"] == NONFINITE).all() and set(r0["exit"]) <= {NONFINITE, CANDIDATE}
    assert c0["candidates"] == int((r0["exit"] == CANDIDATE).sum()) == len(d0)
    twice = [(int(r0["id"][k]), int(r0["best_hd"][k]), float(r0["margin"][k])) for k in range(0, len(r0), 3)]
    assert twice == [(int(r0["id"][k]), int(r0["best_hd"][k]), float(r0["margin"][k])) for k in range(1, len(r0), 3)]   # equal would-be candidates
    assert c1["candidates"] == 2 and c1["duplicates"] == 1 and [d["id"] for d in d1] == [3]
    return {"nonfinite": int((r0["exit"] == NONFINITE).sum()), "equal_pairs_among_them": len(twice), "finite_candidates": c0["candidates"]}


def cond_degenerate(c, reads):
    recs, _ = _all(reads)
    assert list(recs["solved"][:7]) == [0, 0, 0, 1, 1, 1, 1], list(recs["solved"][:7])
    assert (recs["n_wild"][5:] > 0).all() and len(recs) >= 7 + 8
    return {"solved": [int(x) for x in recs["solved"][:7]], "n_wild": [int(x) for x in recs["n_wild"][5:]], "both_nan": int(recs["n_both_nan"].sum())}


def cond_finalize_counts(c, reads):
    out = {}
    for n, (dets, recs, call) in zip(FIN_COUNTS, reads):
        assert call["candidates"] == n and (recs["best_hd"] == 0).all() and len(dets) == min(n, DET_CAP)
        assert [d["id"] for d in dets] == list(range(min(n, DET_CAP)))
        out[n] = len(dets)
    return out


def cond_finalize_dups(c, reads):
    (d0, r0, c0), (d1, r1, c1) = reads
    assert (r0["exit"][:7] == CANDIDATE).all() and list(r0["id"][:7]) == [4] * 5 + [9, 9] and set(r0["rot"][:5]) == {0, 1, 2, 3}
    assert c0["equal_pairs"] >= 1 and c0["duplicates"] >= 4 and [d["id"] for d in d0].count(9) == 2 and [d["id"] for d in d0].count(4) == 1
    nines = [d for d in d0 if d["id"] == 9]
    assert (nines[0]["hamming"], nines[1]["hamming"]) == (0, 1)
    assert list(r0["id"][7:9]) == [12, 12] and [d["id"] for d in d0].count(12) == 1
    assert list(r0["id"][9:11]) == [20, 20] and [d["id"] for d in d0].count(20) == 2 and c0["zero_cross"] >= 1
    assert list(r1["id"]) == [38, 39, 40]
    return {"candidates": c0["candidates"], "duplicates": c0["duplicates"], "equal_pairs": c0["equal_pairs"], "zero_cross": c0["zero_cross"]}


def cond_finalize_two_families(c, reads):
    dets, recs, call = reads[0]
    assert call["candidates"] == 12 and len(dets) == 12 > c["cap"] and sorted(set(d["family"] for d in dets)) == [0, 1]
    return {"candidates": 12, "cap": c["cap"]}


def cond_batch(c, reads, which):
    assert [len(q) for q in c["quads"]] == [0, 1, BATCH_QUAD_CAP] and c["max_batch"] > len(c["frames"])
    if which != "sigma":   # (the filtered frame comes from the device)
        assert [cl["candidates"] for _, _, cl in reads] == [0, 1, BATCH_QUAD_CAP]
    return {"quads": [0, 1, BATCH_QUAD_CAP]}


def measure(oracle, name):
    """The case on the oracle: its conditions asserted, the figures they measured returned."""
    c = case(name)
    _, reads = expected(oracle, c)
    check_truth(c, reads)
    fn, args = CASES[name]
    cond = globals()["cond_" + fn.__name__[5:]]
    return cond(c, reads, *args[:1])


def nan_search(oracle, n=200000, seed=22, chunk=20000):
    """n random quads with integer corners on a 4-pixel grid in 0..64 through the oracle's readout on the degenerate case's frame:
    (quads with a non-finite or out-of-int sample, quads with a sample that is NaN in both coordinates, the first such quad or None)"""
    f = degenerate_frame()
    cfg = config(80, 80, {"families": ["tag36h11"]})
    wild = both = 0
    first = None
    for k in range(0, n, chunk):
        cand = random_grid_quads(seed + k, min(chunk, n - k))
        _, _, recs, _, _ = oracle.decode_trace(f, cfg, [quad(c) for c in cand])
        wild += int((recs["n_wild"] > 0).sum())
        hit = np.flatnonzero(recs["n_both_nan"] > 0)
        both += len(hit)
        if len(hit) and first is None:
            first = cand[hit[0]].tolist()
    return wild, both, first
