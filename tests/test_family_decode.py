"""CPU: tag families beyond the two built-in geometries (tests/family_gen.py) — the bit layout convention, an independent numpy
decoder (np_at3_decode.py) against the oracle, and the oracle against frames drawn by an independent renderer (np_tag_render.py)
at odd bit counts, bits outside the border, reversed borders and 64-bit code words."""
import json
import os
import zlib

import numpy as np
import pytest

import family_gen as fg
import np_at3_decode
import np_tag_render
from chalkydri_amd import default_config, family, synth

HERE = os.path.dirname(os.path.abspath(__file__))
MATRIX = list(fg.MATRIX)
MAX_HAMMING = {"circ21r": 2}          # min_hamming > 2 max_hamming + 1 for every family (3 elsewhere)


def _fam(name):
    return family(name) if name.startswith("tag") else fg.make(name)


def _quarter_turns(fam_p, code):
    """The k of np.rot90(grid(code), k) == grid(rotate90(code)), or None when no quarter turn maps one onto the other."""
    nbits = fam_p.contents.nbits
    g0 = fg.cell_grid(fam_p, code)
    g1 = fg.cell_grid(fam_p, fg.rotate90(np.array([code], np.uint64), nbits)[0])
    ks = [k for k in range(4) if np.array_equal(np.rot90(g0, k), g1)]
    return ks[0] if len(ks) == 1 else None


def test_layout_convention_is_upstreams_and_shared():
    """rotate90 of a code word is one fixed quarter turn of its cell map: for upstream's tag36h11 and tag16h5 layouts and, in the
    same direction, for every generated family."""
    rng = np.random.default_rng(3)
    turns = set()
    for name in ["tag36h11", "tag16h5"] + MATRIX:
        f = _fam(name)
        nbits = f.contents.nbits
        words = [int(c) for c in fg.tables(f)[6][:20]] + [int(v) & ((1 << nbits) - 1) for v in rng.integers(0, 1 << 62, 20) * 4 + 3]
        for w in words:
            k = _quarter_turns(f, w)
            assert k is not None, (name, hex(w))
            turns.add(k)
        # a cell of every data bit, none twice; the centre cell last for odd bit counts
        bx, by = fg.tables(f)[4:6]
        assert len(set(zip(bx.tolist(), by.tolist()))) == nbits
        if nbits % 4 == 1:
            wab = f.contents.width_at_border
            assert (bx[-1], by[-1]) == ((wab - 1) // 2, (wab - 1) // 2)
    assert len(turns) == 1


@pytest.mark.parametrize("name", MATRIX)
def test_generated_codebooks(name):
    nbits, wab, tw, rev, cells, mh, nc = fg.MATRIX[name]
    f = fg.make(name)
    codes = fg.tables(f)[6]
    assert 20 <= len(codes) <= nc and f.contents.min_hamming == mh
    assert all(int(c) < (1 << nbits) for c in codes) and any(int(c) >> (nbits - 1) for c in codes)   # the top bit is used
    rots = [codes]
    for _ in range(3):
        rots.append(fg.rotate90(rots[-1], nbits))
    for i, c in enumerate(codes):
        d = [fg.popcount(r ^ c) for r in rots]
        d[0][i] = 99
        assert min(int(x.min()) for x in d) >= mh, (name, i)


def _pairs_with_oracle(oracle, img, cfg, fams, sharpening=0.25):
    """For every oracle quad: what ora_decode_quads makes of it alone, and what the numpy decoder does, per family."""
    n = 0
    for q in oracle.quads(img, cfg):
        corners = np.array([[q.p[i][0], q.p[i][1]] for i in range(4)])
        want = {d["family"]: d for d in oracle.decode_quads(img, cfg, [q])}
        for fi, f in enumerate(fams):
            if f.contents.reversed_border != q.reversed_border:
                continue
            got = np_at3_decode.decode(img, corners, f, sharpening, cfg.max_hamming)
            assert (got is None) == (fi not in want), (fi, got, want.get(fi))
            if got is None:
                continue
            o = want[fi]
            assert (got["id"], got["hamming"]) == (o["id"], o["hamming"])
            assert np.abs(got["p"] - o["p"]).max() < 1e-9 and np.abs(got["c"] - o["c"]).max() < 1e-9
            assert abs(got["margin"] - o["margin"]) <= 1e-6 * abs(got["margin"])
            n += 1
    return n


GOLDEN = json.load(open(os.path.join(HERE, "golden", "detector_golden.json")))


@pytest.mark.parametrize("g", GOLDEN, ids=[g["case"]["name"] for g in GOLDEN])
def test_np_decoder_matches_oracle_on_golden_scenes(oracle, g):
    """The numpy decoder, checked on a path the suite already trusts (tag36h11, tag16h5)."""
    c = g["case"]
    frame, _ = synth.render(synth.frame_seed(c["seed_cfg"], c["frame"]), c["w"], c["h"], c["n_tags"], tuple(c["families"]), **c["params"])
    assert zlib.crc32(frame.tobytes()) == g["frame_crc32"], "renderer output changed"
    cfg = default_config(c["w"], c["h"], families=tuple(c["families"]), max_hamming=c["bits"], quad_decimate=c["decimate"])
    fams = [family(n) for n in c["families"]]
    assert _pairs_with_oracle(oracle, frame, cfg, fams) >= len(g["detections"]) > 0


def check_truth(dets, truth, floor=40.0, tol=1.0):
    """Every tag whose border is at least `floor` px a side is found with its family and id, corners within tol px, in order."""
    for t in truth:
        tc = t["corners"]
        if min(np.linalg.norm(tc[k] - tc[(k + 1) % 4]) for k in range(4)) < floor:
            continue
        cand = [d for d in dets if (d["family"], d["id"]) == (t["family"], t["id"])]
        assert cand, f"family {t['family']} id {t['id']} missed"
        assert min(np.abs(d["p"] - tc).max() for d in cand) < tol, f"family {t['family']} id {t['id']}: corners off"


@pytest.mark.parametrize("dec", [1, 2])
@pytest.mark.parametrize("name", MATRIX)
def test_oracle_finds_every_family_at_every_rotation(oracle, name, dec):
    f = fg.make(name)
    mh = MAX_HAMMING.get(name, 3)
    n_checked, rots = 0, set()
    for seed in range(3):
        img, truth = np_tag_render.scene([f], 100 * seed + dec, w=643 + 2 * seed, h=481)
        cfg = default_config(img.shape[1], img.shape[0], families=(f,), max_hamming=mh, quad_decimate=dec)
        dets, st = oracle.detect(img, cfg)
        assert st == 0
        check_truth(dets, truth)
        for d in dets:     # (a small code at 2 corrected bits may also be read off a quad that is not a tag)
            assert d["hamming"] == 0 or min(np.abs(d["p"] - t["corners"]).max() for t in truth) > 5
        n_checked += _pairs_with_oracle(oracle, img, cfg, [f])
        for t in truth:
            rots.add(int(np.round(np.rad2deg(np.arctan2(*(t["corners"][1] - t["corners"][0])[::-1])) / 90)) % 4)
    assert n_checked >= 18 and rots == {0, 1, 2, 3}


@pytest.mark.parametrize("name", MATRIX)
def test_bit_errors_up_to_max_hamming(oracle, name):
    """k inverted data cells decode with hamming k for k <= max_hamming; one more and the tag is not reported as its id."""
    f = fg.make(name)
    mh = MAX_HAMMING.get(name, 3)
    assert f.contents.min_hamming > 2 * mh + 1
    for k in range(mh + 2):
        img, truth = np_tag_render.scene([f], 7 + k, flips=k, side=(80, 110))
        cfg = default_config(img.shape[1], img.shape[0], families=(f,), max_hamming=mh)
        dets, _ = oracle.detect(img, cfg)
        for t in truth:
            hit = [d for d in dets if np.abs(d["p"] - t["corners"]).max() < 1.0]
            if k <= mh:
                assert [(d["id"], d["hamming"]) for d in hit] == [(t["id"], k)], (k, t["id"], hit)
            else:
                assert all(d["id"] != t["id"] for d in dets), (k, t["id"])
        _pairs_with_oracle(oracle, img, cfg, [f])


def test_reversed_and_normal_families_side_by_side(oracle):
    """Four families in one configuration, reversed and normal borders mixed, all kinds of tag in the same frames."""
    fams = [family("tag36h11"), fg.make("std41r"), fg.make("circ21r"), fg.make("full64")]
    for seed in range(2):
        img, truth = np_tag_render.scene(fams, 50 + seed, w=961, h=641, cols=4, rows=3)
        cfg = default_config(961, 641, families=tuple(fams), max_hamming=2)
        dets, st = oracle.detect(img, cfg)
        assert st & 15 == 0
        check_truth(dets, truth)
        assert _pairs_with_oracle(oracle, img, cfg, fams) >= len(truth)
