"""The row table of k_emit2's count pass without a device: the exhaustive check of ck_emit_row.h against the definition the kernel
evaluated before (tests/cpp/emit_row_check.cpp, built with AddressSanitizer + UBSan by the Makefile), and the proof, from the
oracle's labels alone, that the frames of tests/emit_row_cases.py put every kind of row at every place the kernel treats differently."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import emit_row_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "chalkydri_amd", "lib", "emit_row_check")


def test_every_reachable_index_of_the_table(built):
    """Six staged words over SKIP and four roots of either colour, times the thread constants: the table entry of every index they
    produce, walked as the kernel walks it, against the earlier kernel's own text; the indices met are the consistent ones."""
    assert os.path.exists(CHECK)
    sym = subprocess.run(["nm", CHECK], capture_output=True, text=True).stdout
    assert "__asan_init" in sym and "__ubsan_handle" in sym          # the build that ran is the sanitized one
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout[-1500:], r.stderr[-2000:])
    print(r.stdout.strip())


@pytest.fixture(scope="module")
def coverage(oracle):
    """(kind, place) -> number of rows over all frames, sizes and gates; and the same for the conditions without their column gate"""
    cover, would = {}, {}
    for w, h in ec.SIZES:
        pl = ec.places(w, h)
        for name, f in ec.frames(w, h).items():
            th, lab, sz = cc.oracle_stages(oracle, f)
            for mcp in ec.MIN_COMPONENT:
                r = ec.rows(th, lab, sz, mcp)
                assert r["leaders"].max() <= 2, (w, h, name, mcp)        # (see emit_row_cases.rim_noise)
                for kn, km in ec.kinds(r).items():
                    for pn, pm in pl.items():
                        cover[(kn, pn)] = cover.get((kn, pn), 0) + int((km & pm).sum())
                for kn in ("would_absorb", "would_drop"):
                    for pn, pm in pl.items():
                        would[(kn, pn)] = would.get((kn, pn), 0) + int((r[kn] & pm).sum())
    return cover, would


# What the definition itself rules out: a row in the last emitting column has no emitting right neighbour to absorb from, one in the
# first none on its left to drop for; and the last column's only partners below min_component_px > 1 are (x-1, y+1) and (x, y+1),
# which touch: one leader at most.
EXCLUDED = {("absorb", "last column"), ("drop", "first column"), ("absorb and drop", "first column"), ("absorb and drop", "last column"),
            ("2 leaders", "last column")}


def test_frames_reach_every_row_kind_at_every_place(coverage):
    """Rows of 0, 1 and 2 leaders, absorbing, dropping and doing both: each inside an emit tile, on a tile seam, and in the first and
    last emitting column and row — every combination but the five the definition excludes, and those must not occur at all, although
    the frames do hold rows in the first column whose 2 x 2 block would merge (the column gate is what says no)."""
    cover, would = coverage
    table = {(k, p): cover.get((k, p), 0) for k in ec.KINDS for p in ec.places(*ec.SIZES[0])}
    print({f"{k} / {p}": n for (k, p), n in table.items()})
    for key, n in table.items():
        assert (n == 0) if key in EXCLUDED else (n > 0), (key, n)
    # (in the last column the (1,1) partner lies in column w - 1, whose pixels are components of one pixel each: no 2 x 2 block
    # with that column has equal words on a diagonal, so the gate on absorb has nothing to refuse)
    assert would[("would_drop", "first column")] > 0


def test_three_leaders_only_at_the_rim_four_nowhere(oracle):
    """Noise at min_component_px = 1 (emit_row_cases.rim_noise): rows of three leaders, all of them in column w - 2, none of four;
    no row of the last column absorbs and none of the first drops."""
    w, h, mcp, named = ec.rim_noise()
    hist, cols = np.zeros(5, np.int64), set()
    for f in named.values():
        th, lab, sz = cc.oracle_stages(oracle, f)
        r = ec.rows(th, lab, sz, mcp)
        hist += np.bincount(r["leaders"].ravel(), minlength=5)
        cols |= set((np.nonzero(r["leaders"] >= 3)[1] + 1).tolist())
        assert not r["absorb"][:, -1].any() and not r["drop"][:, 0].any()
    print("leaders 0..4:", hist.tolist())
    assert hist[3] > 0 and hist[4] == 0 and cols == {w - 2}
