"""The scenes the sub-pixel tests share (test infrastructure, CPU only): the AprilGrid set-up of DESIGN.md §4q — a 4 x 4 tag36h11 board
with corner squares in a 643 x 481 frame, four views, noise of 1.5 to 3.9 grey levels, blur sigma 0 / 0.8 / 1.5 — drawn once per
process, the oracle's detections of them, and ck_detection_t records of oracle detections."""
import functools

import numpy as np

import np_board_render as BR

W, H = 643, 481
BLURS = (0.0, 0.8, 1.5)
SEEDS = (0, 1, 2, 3)


def board():
    from chalkydri_amd.calibration import Board
    return Board(4, 4, 0.088, 0.3, 0)


def _fam():
    from chalkydri_amd import _lib
    return _lib.family("tag36h11")


def noise_of(seed):
    return 1.5 + 0.8 * seed


@functools.lru_cache(maxsize=None)
def board_frame(seed, blur, patched=False):
    """(frame, truth) of view `seed`; patched: a flat grey patch lies on the board over the four middle tags, reaching half a gap past
    their outer corners"""
    patch = None
    if patched:
        b = board()
        lo, hi = b.pitch - 0.5 * b.tag_size * b.tag_spacing, 3 * b.pitch - 0.5 * b.tag_size * b.tag_spacing
        patch = BR.board_patch(BR.board_homography(b.rows, b.cols, b.tag_size, b.tag_spacing, W, H, seed), lo, lo, hi, hi)
    return BR.render(_fam(), seed=seed, blur=blur, noise=noise_of(seed), patch=patch)


@functools.lru_cache(maxsize=None)
def board_dets(seed, blur, patched=False):
    """the oracle's detections of that frame (list of dicts)"""
    import pyoracle
    from chalkydri_amd import default_config
    return pyoracle.detect(board_frame(seed, blur, patched)[0], default_config(W, H))[0]


def records(dets):
    """oracle detections (dicts) -> list of ck_detection_t"""
    from chalkydri_amd import _abi as A
    out = []
    for d in dets:
        r = A.Detection()
        r.id, r.hamming, r.family, r.decision_margin = d["id"], d["hamming"], d["family"], d["margin"]
        r.c[0], r.c[1] = d["c"]
        for k in range(4):
            r.p[k][0], r.p[k][1] = d["p"][k]
        out.append(r)
    return out


def seeds_of(dets, n_tags=16):
    """the detections that may seed the board: hamming 0, an id on the board, the first per id"""
    seen, out = set(), []
    for d in dets:
        if d["hamming"] == 0 and d["family"] == 0 and 0 <= d["id"] < n_tags and d["id"] not in seen:
            seen.add(d["id"])
            out.append(d)
    return out


def rms(e):
    e = np.asarray(e, float).reshape(-1, 2)
    return float(np.sqrt((e ** 2).sum(1).mean()))
