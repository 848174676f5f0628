"""The cases of tests/test_gpu_span_alignment.py are not vacuous: with the oracle alone (no GPU), every frame of tests/span_cases.py is
shown to hold what it is pinned at, on the oracle's per-cluster readout, and the bases of the sweep are shown to put a cluster on
every edge of the split fit's grid that span_cases.placement names.  Where a condition fails, the INPUT is what changes: the
conditions are the cases' meaning.

Measured when the cases were written (default settings; every sweep frame: one cluster at the fit, which becomes the frame's one quad):

  frame       points after duplicate removal, ksz, maxima      frame       points, ksz, maxima
  small_64      64   5    4                                    clean_240   2016  20  100
  small_120    120  10    7                                    clean_300   2520  20  126
  small_232    232  19   11                                    edge_64      808  20   64
  small_240    240  20   14                                    edge_65      792  20   65
  clean_40     336  20   12                                    edge_256    2520  20  256
  clean_80     672  20   28                                    edge_257    2560  20  257
  clean_120   1008  20   46                                    beyond      3360  20  322   (the 448 sheet; all others 352)
  clean_160   1344  20   64

  sizes <= 911: 8 frames; in [960, 1871]: 2; >= 1922: 5; >= 2880: 1.  Maxima <= 64: 9 frames; 65 .. 256: 4; > 256: 2.
  Bases 0 .. 1023 reach, in every size group, each of e0 % 32 == 0, e0 % 960 in {0, 1, 959}, es == 0, e1 % 960 in {0, 1},
  (es + sz + 49) % 960 in {0, 1}, both numbers of spans a cluster of the group can touch (1 | 2, 2 | 3, 3 | 4, 4 | 5), and the heads'
  prefetch as well as the run tables in the two groups of up to 1871 points (the run tables alone beyond: three runs and more).
  crowded frames (640x480): 451 and 391 clusters at the fit, 128 536 and 122 575 live positions (condition: > 15 360) = 134 and 128
  spans for 8 workgroups, 27 and 36 quads.
"""
import os
import re

import numpy as np
import pytest

import span_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sweep(oracle):
    return sc.CONDITIONS["sweep"](oracle)


def test_sweep_frames_are_single_quad_clusters_of_the_pinned_size(sweep):
    """One row with EXIT >= 6 per frame, a quad, of the pinned points, ksz and maxima (check_sweep asserts; the figures are printed)."""
    fig, quads = sweep
    print(fig)
    assert [len(quads[s]) for s in sc.SHEETS] == [len(sc.sweep_rows(s)) for s in sc.SHEETS] == [14, 1]
    assert all(len(q) == 1 for s in sc.SHEETS for q in quads[s])
    assert max(sc.SHEETS) <= 480


def test_sizes_and_maxima_cover_their_groups(sweep):
    fig, _ = sweep
    sizes = [r[3] for r in sc.SWEEP]
    assert any(s <= 911 for s in sizes) and any(960 <= s <= 1871 for s in sizes) and any(s >= 1922 for s in sizes) and any(s >= 2 * 960 + 960 for s in sizes)
    found = [r[5] for r in sc.SWEEP]
    assert any(n <= 64 for n in found) and any(65 <= n <= 256 for n in found) and any(n > 256 for n in found)
    assert {64, 65, 256, 257} <= set(found)
    # (the groups of span_cases are these intervals)
    assert [len(fig["sizes, " + g]) for g, _ in sc.SIZE_GROUPS] == [sum(s <= 911 for s in sizes), sum(960 <= s <= 1871 for s in sizes),
                                                                    sum(s >= 1922 for s in sizes), sum(s >= 2880 for s in sizes)]
    # the window half-width travels in the point word: ksz = points / 12 below 240 points
    assert all(r[4] == min(r[3] // 12, 20) for r in sc.SWEEP) and {5, 10, 19, 20} <= set(r[4] for r in sc.SWEEP)
    assert any(r[3] == 240 for r in sc.SWEEP) and any(228 <= r[3] <= 236 for r in sc.SWEEP)


@pytest.mark.parametrize("group", [g for g, _ in sc.SIZE_GROUPS])
def test_bases_reach_every_edge_in_every_size_group(group):
    cond = dict(sc.SIZE_GROUPS)[group]
    reached = set()
    for _, _, _, sz, _, found in sc.SWEEP:
        if cond(sz):
            reached |= sc.edges_possible(sz, found)
    missing = sc.edges_required(group) - reached
    assert not missing, (group, sorted(missing))


def test_placement_names_the_edges():
    """placement() on placements worked out by hand."""
    assert sc.placement(64, 4, 0) >= {"es == 0", "spans touched: 1", "heads prefetch"}
    assert "e0 % 32 == 0" in sc.placement(64, 4, 7) and "e0 % 32 == 0" not in sc.placement(64, 4, 8)
    assert "e0 % 960 == 0" in sc.placement(64, 4, 935) and "e0 % 960 == 959" in sc.placement(64, 4, 934) and "e0 % 960 == 1" in sc.placement(64, 4, 936)
    assert sc.placement(64, 4, 934) >= {"spans touched: 2"} and sc.placement(64, 4, 935) >= {"spans touched: 1"}
    assert "e1 % 960 == 0" in sc.placement(336, 12, 599) and "e1 % 960 == 1" in sc.placement(336, 12, 600)
    assert "end % 960 == 0" in sc.placement(336, 12, 575) and "end % 960 == 1" in sc.placement(336, 12, 576)
    assert "run tables" in sc.placement(792, 65, 0) and "heads prefetch" in sc.placement(808, 64, 500)
    assert sc.placement(1008, 46, 0) >= {"spans touched: 2", "heads prefetch"} and sc.placement(1008, 46, 900) >= {"spans touched: 3", "run tables"}
    assert "spans touched: 5" in sc.placement(3360, 322, 500) and "spans touched: 4" in sc.placement(3360, 322, 0)


def test_bases_of_the_poisoned_and_loop_runs():
    assert set(sc.POISON_BASES) == set(range(128)) | set(range(896, 1024)) and set(sc.POISON_BASES) <= set(sc.BASES)
    assert sc.LOOP_BASES == (0, 1, 31, 935, 959, 960) and max(sc.BASES) <= sc.BASE_MAX
    # around span 0's start and the first span boundary: es == 0 and every residue e0 % 960 of {959, 0, 1} are among them
    got = set()
    for b in sc.POISON_BASES:
        got |= sc.placement(336, 12, b)
    assert got >= {"es == 0", "e0 % 960 == 959", "e0 % 960 == 0", "e0 % 960 == 1", "e0 % 32 == 0"}


def test_crowded_frames_give_every_workgroup_several_spans(oracle):
    fig, quads = sc.CONDITIONS["crowded"](oracle)
    print(fig)
    assert sc.CROWDED_MIN == 2 * 8 * 960 == 15360 and len(quads) == 2
    for i in range(2):
        spans = fig["frame %d" % i]["spans"]
        assert spans // sc.LOOP_WGS >= 2 and -(-spans // sc.LOOP_WGS) >= 3   # every workgroup takes two spans at least, some take three


def test_cases_know_the_kernels_constants():
    csrc = os.path.join(ROOT, "chalkydri_amd", "csrc")
    src = open(os.path.join(csrc, "k_quads.hip")).read()
    chunk = open(os.path.join(csrc, "k_chunk.hip")).read()
    hdr = open(os.path.join(csrc, "ck_internal.h")).read()
    assert int(re.search(r"constexpr int CK_SPAN = (\d+);", hdr).group(1)) == sc.SPAN
    m = re.search(r"constexpr int CK_EXT_PRE = (\d+), CK_EXT_POST = (\d+),", hdr)
    assert (int(m.group(1)), int(m.group(2))) == (sc.EXT_PRE, sc.EXT_POST)
    assert int(re.search(r"constexpr int KL = 1024, KOFF = (\d+);", chunk).group(1)) == sc.KOFF
    # the knob: clamped to the room the diagnostics build adds to a frame, and that room is the diagnostics build's alone
    assert re.search(r"if \(ext_base > 2 \* CK_SPAN\) ext_base = 2 \* CK_SPAN;", chunk) and sc.BASE_MAX == 2 * sc.SPAN
    stages = open(os.path.join(csrc, "ck_stages.hip")).read()
    assert re.search(r"int ck_ext_room\(\) \{\n#ifdef CK_DIAG\n\s*return 2 \* CK_SPAN;\n#else\n\s*return 0;\n#endif\n\}", chunk)
    assert re.search(r"e \+= \(size_t\)ck_ext_room\(\);", stages) and "CK_DIAG" not in stages and "CK_DIAG" not in src
    # k_chunk's workgroups per frame in the loop test: the grid's minimum
    assert re.search(r"if \(gx < (\d+)\) gx = \1;", chunk).group(1) == str(sc.LOOP_WGS)
