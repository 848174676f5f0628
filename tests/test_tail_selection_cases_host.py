"""The cases of tests/test_gpu_tail_selection.py are not vacuous: with the oracle alone (no GPU), every case of
tests/tail_selection_cases.py is shown to hold what it is named for, on the oracle's per-cluster readout (maxima found and kept, points
after duplicate removal, where the cluster leaves the fit).  The figures are printed per case (pytest -s shows them).  Where a condition
fails, the INPUT is what changes: the conditions are the cases' meaning.

Measured when the cases were written (condition: minimum -> measured, max_nmaxima 4 / 10 / 12):

  edges_m4 / _m10 / _m12    quads from clusters of exactly 64, 65, 256 and 257 maxima      1 each  1 each
                            clusters of 65 .. 256 maxima; of them cut to max_nmaxima          10   34; 34 (337 clusters in the five frames)
                            of them in three or more spans (>= 1922 points); and quads         1   8; 1
                            clusters of <= 64 maxima and more than max_nmaxima                10   256 / 154 / 122
                            quads                                                              5   5 / 15 / 16
  beyond_m10                quads from clusters of >= 296 maxima                               1   1 (322 maxima)
  ties_m10 / _m12           quads from clusters of 65 .. 256 maxima that kept < max_nmaxima    1   2 (of 94 and 78 maxima, kept 8 and 6) / 1 (of 94, kept 10)
"""
import os
import re

import numpy as np
import pytest

import quad_cases as qc
import tail_selection_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_meets_its_conditions(oracle, name):
    figures, quads, index, rd = tc.measure(oracle, name)
    print(name, figures)
    frames, settings, _ = tc.case(name)
    assert len(index) == len(frames) and set(index) == set(quads)
    assert settings["max_nmaxima"] in tc.NMAXIMA
    assert max(frames.shape[1:]) <= 512   # (a few hundred pixels a side: the device runs take seconds)


def test_edge_squares_are_single_clusters_of_the_pinned_size(oracle):
    """Each square of EDGES alone on its sheet: one cluster, of exactly the pinned number of maxima, a quad under every setting."""
    frames, _, _ = tc.case("edges_m10")
    for (side, seed, n), f in zip(tc.EDGES, frames):
        for m in tc.NMAXIMA:
            rd, quads = qc.trace(oracle, f, {"max_nmaxima": m})
            assert len(rd) == 1 and rd[0, qc.FOUND] == n and rd[0, qc.KEPT] == m and rd[0, qc.EXIT] == qc.QUAD and len(quads) == 1, (side, seed, rd)


def test_cases_know_the_kernels_constants():
    src = open(os.path.join(ROOT, "chalkydri_amd", "csrc", "k_quads.hip")).read()
    hdr = open(os.path.join(ROOT, "chalkydri_amd", "csrc", "ck_internal.h")).read()
    assert int(re.search(r"constexpr int SEL_RV = (\d+);", src).group(1)) == tc.RV
    assert int(re.search(r"constexpr int CK_SPAN = (\d+);", hdr).group(1)) == tc.SPAN
    assert np.array_equal([n for _, _, n in tc.EDGES], [64, 65, 64 * tc.RV, 64 * tc.RV + 1])
