"""The cases of tests/decode_cases.py reach the edges they are named for: asserted on the oracle's per-(quad, family) readout
(ora_decode_last, pyoracle.decode_trace), without a GPU.  What was reached (figures of the readout):

    case                    what the readout shows
    search_t36n767..2115    every drawn id at distance 0, one pair only; ids 5 | 766 ; 5, 767 ; 5, 767, 768 ; .., 1535, 1536 ; .., 2114:
    search_f64n767..2115      the last id of a pass, the first of the next, the very last (tag36h11's 36-bit and full64's 64-bit layout)
    ties_sym                ids 0 (all black) and 1 (all white): 4 pairs at distance 0, rotation 0 chosen, margin exactly 0.0, accepted
    ties_dup                one code at ids 3 and 800 (second pass): 2 pairs at distance 0, id 3 chosen
    ties_rot                word 0x5A3C96E1B: (rotation 0, id 700) and (rotation 1, id 2) both at distance 2; rotation 0, id 700 chosen
    hamming_0 / hamming_3   best distances 0, 1, 0, 1 / 3, 4, 3, 4: candidate, rejected, candidate, rejected
    sharpen_0 / 025 / 1     total_width 9, 10 (reversed border) and 16, two bits flipped each; margins 85 / 87 / 87, 168 / 184 / 166,
                            412 / 477 / 402
    overhang_even / odd     28 / 30 tags over the four sides by 0..12 / 1..13 px (and 7.4): border samples in (-1, 0), [w - 1, w) and
                            [w, w + 1), bit samples on pixel centres, within half a pixel of the last column and skipped just beyond
                            it; 23 of 28 / 23 of 30 decode, 7 / 7 of them with bit samples outside the frame
    posed                   six tags turned 17..324 degrees and tilted, normal and reversed border: six candidates at distances 0 x 5 and 2, no
                            corner coordinate a multiple of 1/1024; the other family leaves at the border sense
    model                   exits margin (NaN) x 3; white model NaN, both NaN, white NaN; border samples used 0 + 32, 0 + 0, 6 + 6; every
                            bit sample inside; nothing comes back; the whole-frame quad with a reversed border (std41r) leaves
                            through the sign test on its NaN white model
    model_strip             a 96 x 16 frame between the samples of a sheared quad: 1 white sample, 0 black ones, 1 bit inside; black
                            model NaN, exit margin (NaN)
    degenerate              four equal corners, four collinear corners, bow-tie: singular; two coincident corners, three collinear
                            corners, the two integer quads with zz == 0: solved; samples with a non-finite coordinate per quad
                            2, 2, then 2, 1, 9, 1, 1, 3, 1, 4, 1, 1, 1, 1 in the hits of the seeded search
    finalize_counts         255, 256, 257, 300 candidates -> 255, 256, 256, 256 detections (ids 0..255), overflow from 257 on
    finalize_dups           11 candidates, 5 duplicates dropped, 10 pairs equal in (family, id, hamming, float margin), 2 cross products
                            exactly zero (on the line of an edge, outside the quad: not decisive); id 9 twice (hamming 0 before hamming 1), ids 4 and 12 once, id 20 twice; ids 38, 39, 40
    finalize_edge           two quads over one black rectangle, both id 0 at margin 0.0; each centre exactly on an edge of the other:
                            one cross product 0, the three others of one sign, in both directions; 1 duplicate dropped, 1 kept
    finalize_nan            ZZ quads and seeded hits under tag16h5 at max_hamming 3, each twice and cycled: 15 records decode with a
                            non-finite corner (exit 6), 6 equal pairs among them, no candidate from them; 3 cycled copies read with
                            finite corners and are candidates; a drawn tag twice on a second frame: 2 candidates, 1 kept
    finalize_two_families   12 candidates of 6 quads, caller's cap 5
    batch_plain/dec2/sigma  0, 1 and quad_cap = 32 quads on a handle of 6 frames

No sample that is NaN in BOTH coordinates was found: 200 000 random quads with integer corners on a 4-pixel grid in 0..64 (seed 22)
hold 14 215 with a non-finite or out-of-int sample coordinate and none with both coordinates NaN (xx = yy = zz = 0 would need a
singular H, which the elimination refuses)."""
import numpy as np
import pytest

import decode_cases as dc


@pytest.mark.parametrize("name", dc.NAMES)
def test_case_reaches_its_edge(oracle, name):
    figures = dc.measure(oracle, name)
    print(name, figures)
    c = dc.case(name)
    n, h, w = c["frames"].shape
    assert w <= 420 and h <= 400 and len(c["quads"]) == n == len(c["truth"])
    cap = c["settings"].get("max_quads_per_frame", 1024)
    assert all(len(q) <= cap for q in c["quads"])


def test_no_sample_is_nan_in_both_coordinates(oracle):
    """the bounded search the degenerate case's docstring speaks of"""
    wild, both, first = dc.nan_search(oracle)
    print(wild, both, first)
    assert wild > 10000 and both == 0, first


def test_readout_agrees_with_the_decode(oracle):
    """decode_trace returns decode_quads' detections; one record per (quad, family); the candidates are the records that left at 5,
    and a record's id, distance and margin are its candidate's."""
    c = dc.case("finalize_two_families")
    f = c["frames"][0]
    cfg = dc.config(f.shape[1], f.shape[0], c["settings"])
    plain = oracle.decode_quads(f, cfg, c["quads"][0])
    dets, raw, recs, call, ov = oracle.decode_trace(f, cfg, c["quads"][0])
    assert len(raw) == 96 * len(dets) and not ov
    assert [(d["id"], d["hamming"], d["margin"], d["p"].tobytes()) for d in plain] == [(d["id"], d["hamming"], d["margin"], d["p"].tobytes()) for d in dets]
    assert len(recs) == len(c["quads"][0]) * 2 and list(recs["family"]) == [0, 1] * len(c["quads"][0])
    assert call["candidates"] == int((recs["exit"] == dc.CANDIDATE).sum()) == len(dets) + call["duplicates"]
    got = sorted((int(r["family"]), int(r["id"]), int(r["best_hd"]), float(np.float32(r["margin"]))) for r in recs)
    assert got == sorted((d["family"], d["id"], d["hamming"], d["margin"]) for d in dets)


def test_range_rule_skips_what_no_int_holds(oracle):
    """The two integer quads whose zz is 0 at border samples: the samples are skipped (62 of 64 used), whatever their conversion to int
    would have given."""
    c = dc.case("degenerate")
    _, reads = dc.expected(oracle, c)
    recs = reads[0][1]
    for k in (5, 6):
        assert recs["n_wild"][k] == 2 and recs["n_white"][k] + recs["n_black"][k] <= 62 and recs["solved"][k] == 1
