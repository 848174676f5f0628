"""CPU: the premise of the quad fit's distinct-points path (k_quads.hip: FitArgs::distinct), on the oracle's clusters alone.  The only
coordinates a cluster holds twice are the diagonal twins k_emit2 stores as one word: after the merge a cluster's stored points are
its distinct coordinates, no two sort keys are equal, and the fit needs neither the tie-break of its rank sort nor the search for
duplicates behind it.  Checked on every frame of the twin-point and row-table tests and on a noise frame, against a numpy
restatement of where the emission rule doubles a coordinate (tests/fit_distinct_cases.py: twin_positions)."""
import numpy as np
import pytest

import cluster_cases as cc
import fit_distinct_cases as fd


@pytest.fixture(scope="module")
def survey(oracle):
    """one pass over all frames: the assertions per frame, and what the frames reach together"""
    reach = dict(seam_x=0, seam_y=0, col_first=0, col_last=0, short=0, doubles=0, frames=0, clusters=0)
    for name, frame, mcp in fd.host_frames():
        h, w = frame.shape
        (th, lab, sz), keys, counts, (ci, x, y, gx, gy) = fd.cluster_points(oracle, frame, mcp)
        reach["frames"] += 1
        reach["clusters"] += len(keys)
        tk, tx, ty = fd.twin_positions(th, lab, sz, mcp)
        if not len(ci):
            assert not len(tk), name
            continue
        assert np.all(keys[1:] > keys[:-1]), name   # (the oracle files its clusters by key)
        # every stored point as (cluster, x, y): how often each occurs
        code = (ci << 32) | (x << 16) | y
        order = np.argsort(code, kind="stable")
        ucode, first, n = np.unique(code[order], return_index=True, return_counts=True)
        assert n.max() <= 2, f"{name}: a coordinate {n.max()} times in one cluster"
        dbl = ucode[n == 2]
        dx, dy = (dbl >> 16) & 0xFFFF, dbl & 0xFFFF
        assert np.all(dx & 1) and np.all(dy & 1), f"{name}: a double that is not an (odd, odd) half-pixel"
        # ... and its two copies are the (1,1) point of one pixel and the (-1,1) point of its right neighbour: gradients (s, s) and (-s', s')
        at = first[n == 2]
        g0x, g0y, g1x, g1y = gx[order][at], gy[order][at], gx[order][at + 1], gy[order][at + 1]
        assert np.all(np.abs(np.stack([g0x, g0y, g1x, g1y])) == 1) and np.all(g0x * g0y + g1x * g1y == 0), name
        # ... and the doubles are exactly the twin positions of the restated rule, cluster by cluster
        tci = np.searchsorted(keys, tk)
        assert np.all(tci < len(keys)) and np.array_equal(keys[tci], tk), f"{name}: a twin position in no cluster"
        tcode = np.sort((tci.astype(np.int64) << 32) | (tx.astype(np.int64) << 16) | ty.astype(np.int64))
        assert np.array_equal(tcode, dbl), f"{name}: {len(dbl)} doubled coordinates, {len(tcode)} twin positions"
        distinct = np.bincount(ucode >> 32, minlength=len(keys))
        assert np.array_equal(counts - distinct, np.bincount(tci, minlength=len(keys))), name
        px, py = (dx - 1) // 2, (dy - 1) // 2   # the pixel whose (1,1) point it is
        reach["doubles"] += len(dbl)
        reach["seam_x"] += int(np.count_nonzero((px % cc.ETW == cc.ETW - 1) & (px + 1 <= w - 2)))
        reach["seam_y"] += int(np.count_nonzero(py % cc.ETH == cc.ETH - 1))
        reach["col_first"] += int(np.count_nonzero(px == 1))
        reach["col_last"] += int(np.count_nonzero(px == w - 3))   # its partner is the last emitting column, w - 2
        reach["short"] += int(np.count_nonzero((counts >= 24) & (distinct < 24)))
    return reach


def test_only_twins_come_twice(survey):
    """(the assertions stand in the survey; here: that it saw enough to mean something)"""
    assert survey["frames"] >= 240 and survey["clusters"] >= 5000 and survey["doubles"] >= 10000, survey


def test_frames_reach_the_places_where_the_merge_could_fail(survey):
    """doubles whose two owners sit in different emit tiles (x = 63 | 64 and y = 15 | 16 of a 64 x 16 tile), doubles owned by the first
    and by the last emitting column, and clusters that pass the size gate of 24 points with fewer than 24 distinct coordinates"""
    for k in ("seam_x", "seam_y", "col_first", "col_last", "short"):
        assert survey[k] > 0, (k, survey)
