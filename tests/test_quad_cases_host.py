"""The cases of tests/test_gpu_quad_back.py are not vacuous: with the oracle alone (no GPU), every case of tests/quad_cases.py is shown
to reach the edge of the quad fit's back half it is named for, on the oracle's per-cluster readout (pyoracle.fit_trace: where the
cluster leaves fit_quad, its points before and after duplicate removal, ksz, maxima found and kept, 4-subsets tied for the best energy,
border direction).  The figures are printed per case (pytest -s shows them).  Where a condition fails, the INPUT is what changes: the
conditions are the cases' meaning.

Measured when the cases were written (condition: minimum -> measured):

  case                      condition                                                   min   measured
  small                     ksz == 2                                                      5   66
                            exactly 24 points after duplicate removal                     1   22
                            >= 24 points before, < 24 after (exit 5)                      1   7
                            exit 6                                                        1   14
                            clusters with 2 / 3 / 4 maxima                            1 each  4 / 10 / 52
                            quads                                                        10   123
  mse_window_0 / _1 / _2    exit 8 (clusters of 60; 32, 32, 32, 32; 88 points)            1   1 / 4 / 1
  noise, quad_decimate 1    nmax == max_nmaxima        (max_nmaxima 4 / 10 / 12)          1   1 / 68 / 46
                            nmax == max_nmaxima + 1                                       1   4 / 50 / 40
                            nmax >= 65 (largest 215); ksz == 20                           1   26; 197
                            exit 7                                                        1   219 / 35 / 33
                            exit 10                                                       1   4 / 3 / 2
                            exit 11                                                       1   347 / 366 / 350
                            exit 12                                                       1   82 / 165 / 190
                            exit 13                                                       1   70 / 148 / 136
                            quads                                                         5   28 / 33 / 39
  noise, quad_decimate 2    nmax == max_nmaxima; + 1                                      1   1 / 8 / 14; 6 / 17 / 3
                            nmax >= 65 (largest 109); ksz == 20                           1   6; 30
                            exits 7; 10; 11; 12; 13                                       1   46 / 9 / 8; 1 / 1 / 1; 23 / 6 / 5; 18 / 53 / 51; 37 / 53 / 54
                            quads                                                         5   31 / 34 / 37
  noise cos_critical 0.5    as max_nmaxima 10, decimate 1, but exits 7; 12; 13; quads         122; 273; 16; 11
  ties_m9 / _m10 / _m11     more maxima than the cut, kept < max_nmaxima                  1   2 / 2 / 3   (of 71 / 62 / 52 past the cut)
                            quads from clusters with >= 2 subsets of bit-equal energy     1   1 / 2 / 2   (the tie WAS found, so it is required)
  border_d1 / _d2           quads with a corner < quad_decimate + 1 px from the border    1   1 (1.0 px; four more at 2.0) / 2 (2.5 px)
  long; reversed            longest edge > 136 px; quads with reversed_border = 1         1   160.2 px; 1
  batch_d1 / _d2            frames (5 distinct); quads in the distinct frames            10   40; 156 / 68
  classes_d1 / _d2          quads, refine_edges 1, from a cluster of 64 / 128 / 256 / 512
                            threads (17 / 33 copies of one 361x396 / 722x792 frame)   1 each  1 / 1 / 1 / 1  (436, 728, 1460, 4102 points)
  (refine_edges does not enter the readout: the r0 and r1 cases of a noise setting measure the same.)

Why classes_*: k_fit runs a cluster on 64 (up to 512 points), 128 (513..1024), 256 (1025..4096) or 512 threads (more), and what only a
workgroup of several waves does (a pair fit per lane, reductions and a broadcast across waves) needs a cluster that goes all the way
to a refined quad at each.  Quads per thread count (qc.quads_per_thread_count) in the cases that have refine_edges on, before classes_*:
  64: every case but long / reversed; 128: noise_*_d1 3..6, noise_m12_d2 1, border_d1 9, batch_d1 5 — in calls of 3 frames, which do
  without the 128-thread class, all but batch_d1's; 256: noise_m12_d1 1, long 1, reversed 1; 512: none; quad_decimate 2: 256 and 512 none.
  tests/test_gpu_seq_front.py's nested quadrilaterals (default settings): edges640 1 / 1 / 2 / 0, edges272 2 / 1 / 1 / 0, shapes640 5 / 1 / 0 / 0.
"""
import numpy as np
import pytest

import quad_cases as qc


@pytest.fixture(scope="module")
def measured(oracle):
    """name -> (figures, quads, index, readouts), each case traced once"""
    return {}


def _measure(oracle, measured, name):
    if name not in measured:
        measured[name] = qc.measure(oracle, name)
    return measured[name]


@pytest.mark.parametrize("name", qc.NAMES)
def test_case_meets_its_conditions(oracle, measured, name):
    """qc.measure asserts the case's conditions (the minimums of its check function) and that no cluster leaves at exit 9."""
    figures, quads, index, rd = _measure(oracle, measured, name)
    print(name, figures)
    frames, settings, _ = qc.case(name)
    assert len(index) == len(frames) and set(index) == set(quads)
    assert not (rd[:, qc.EXIT] == 9).any()


def test_readout_agrees_with_the_fit(oracle):
    """fit_trace gives the oracle one cluster at a time: the quads are the ones ora_fit_quads returns for the whole frame, bit for bit,
    the exits add up to what ora_fit_stats counts, and the fields are consistent with each other."""
    import ctypes as C
    import cluster_cases as cc
    frames, settings, _ = qc.case("noise_m10_d1_r1")
    frame = frames[0]
    h, w = frame.shape
    cfg = qc.config(w, h, settings)
    th, lab, sz = cc.oracle_stages(oracle, frame, 1, cfg.min_white_black_diff)
    cl, pts, _ = oracle.clusters(th, lab, sz, cfg.min_component_px)
    stats = (C.c_long * 16)()
    oracle.lib().ora_fit_stats(stats, 1)
    whole = qc.sort_quads(oracle.quads_to_np(oracle.fit_quads(frame, cfg, cl, pts)[0]))
    oracle.lib().ora_fit_stats(stats, 1)
    rd, one_by_one = qc.trace(oracle, frame, settings)
    assert len(whole) >= 5 and np.array_equal(whole, one_by_one)
    assert len(rd) == len(cl) == stats[0]
    for k in range(1, 15):
        assert int((rd[:, qc.EXIT] == k).sum()) == stats[k], k
    assert np.array_equal(rd[:, qc.POINTS], cl[:, 3].astype(np.int64))
    past = lambda k: rd[:, qc.EXIT] > k
    assert (rd[~past(4), qc.UNIQUE] == -1).all() and (rd[past(4), qc.UNIQUE] >= 1).all() and (rd[past(4), qc.UNIQUE] <= rd[past(4), qc.POINTS]).all()
    assert np.array_equal(rd[past(5), qc.KSZ], np.minimum(rd[past(5), qc.UNIQUE] // 12, 20))
    assert (rd[past(6), qc.FOUND] >= 4).all() and (rd[rd[:, qc.EXIT] == 6, qc.FOUND] < 4).all()
    m = settings["max_nmaxima"]
    assert np.array_equal(rd[past(6), qc.KEPT] == rd[past(6), qc.FOUND], rd[past(6), qc.FOUND] <= m) and (rd[past(6), qc.KEPT] <= m).all()
    assert (rd[rd[:, qc.EXIT] == 7, qc.TIES] == 0).all() and (rd[past(7), qc.TIES] >= 1).all()
    assert set(rd[past(3), qc.REVERSED].tolist()) <= {0, 1} and (rd[rd[:, qc.EXIT] == qc.QUAD, qc.REVERSED] == 0).all()   # tag36h11: normal borders only


def test_mse_window_is_where_the_formula_puts_it(oracle):
    """A cluster of sz points leaves at exit 8 when each of its four lines passes (mse <= max_mse) and their summed error over sz does not:
    the same clusters become quads under a bound a little wider, which is what makes the window an edge and not a different input."""
    for k, (v, which) in enumerate(qc.MSE_WINDOW):
        frames, settings, _ = qc.case("mse_window_%d" % k)
        assert settings["max_line_fit_mse"] == v
        for f in frames:
            rd, _ = qc.trace(oracle, f, settings)
            wide, _ = qc.trace(oracle, f, dict(settings, max_line_fit_mse=v * 1.5))
            at8 = rd[:, qc.EXIT] == 8
            assert at8.any() and (wide[at8, qc.EXIT] > 8).all()


def test_batch_is_the_small_and_noise_frames(oracle):
    frames, settings, _ = qc.case("batch_d1")
    assert frames.shape == (qc.BATCH_FRAMES, qc.SMALL_H, qc.SMALL_W) and (qc.NOISE_W, qc.NOISE_H) == (qc.SMALL_W, qc.SMALL_H)
    assert set(settings) == {"quad_decimate"}   # default settings otherwise
    assert len(set(qc.frame_index(frames))) == 5
