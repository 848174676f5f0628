"""The cases of tests/test_gpu_clusters.py are not vacuous: with the oracle alone (no GPU), every case is shown to reach the edge of
k_clusters.hip it is named for — how many clusters k_scan keeps, how many component pairs meet in one 64 x 16 emit tile, how many
(tile, pair) runs k_scatter copies and how long they are, the exact cluster and component sizes at the gates.  The figures are
printed per case (pytest -s shows them).  Where a condition fails, the INPUT is what changes: the conditions are the cases' meaning."""
import numpy as np
import pytest

import cluster_cases as cc


def _stats(oracle, img, min_component_px, dec=1, min_cluster_pixels=24):
    th, lab, sz = cc.oracle_stages(oracle, img, dec)
    return cc.emit_stats(th, lab, sz, min_component_px, min_cluster_pixels), (th, lab, sz)


@pytest.mark.parametrize("kind,w,h,mcp", [("noise", 130, 49, 5), ("blobs", 191, 63, 25), ("tags", 258, 98, 5), ("spiral", 129, 33, 25), ("stripes", 66, 33, 1)])
def test_emit_stats_agree_with_the_oracle(oracle, kind, w, h, mcp):
    """The numpy restatement of the emit rule counts what the oracle counts: the same number of clusters, of the same sizes, and
    every point in exactly one (tile, pair) run."""
    img = cc.frame(kind, w, h, 7)
    s, (th, lab, sz) = _stats(oracle, img, mcp)
    cl, pts, ov = oracle.clusters(th, lab, sz, mcp)
    assert not ov and len(cl) == s.pairs and len(cl) > 0
    assert sorted(int(c) for c in cl[:, 3]) == sorted(int(c) for c in s.cluster_sizes)
    lo, hi = cc.gate(w, h)
    assert s.kept == sum(1 for c in cl[:, 3] if lo <= c <= hi)
    assert int(s.pairs_per_tile.sum()) == s.runs and s.runs >= s.pairs
    assert int(s.run_lengths.sum()) == sum(int(c) for c in cl[:, 3] if lo <= c <= hi)


def test_geometry_cases(oracle):
    """a: every noise and blobs frame keeps at least 3 clusters; over the matrix the kept clusters' runs fall into each of the bins
    1..16, 17..64, 65..256 and >= 257, and runs of exactly 16, 17, 64, 65, 256 and 257 points all occur; the sizes are the ragged
    ones they are listed as."""
    total, edges = np.zeros(4, np.int64), set()
    for w, h, dec in cc.GEOMETRY:
        for kind in cc.geometry_kinds(w, h, dec):
            fr = cc.geometry_frames(w, h, kind)
            assert len({f.tobytes() for f in fr}) == (1 if kind in ("stripes", "spiral") else cc.GEOMETRY_N)   # drawn kinds have no seed
            for mcp in cc.GEOMETRY_MIN_COMPONENT:
                for i, f in enumerate(fr):
                    s, _ = _stats(oracle, f, mcp, dec)
                    print(f"a {w}x{h}/{dec} {kind} min_component_px={mcp} frame {i}: {s.line()}")
                    if kind in ("noise", "blobs"):
                        assert s.kept >= 3, (w, h, dec, kind, mcp, i, s.kept)
                    if kind == "noise" and (w, h) == (130, 49) and mcp == 5:
                        assert all(b > 0 for b in s.bins())   # this one frame size has every bin on its own
                    total += s.bins()
                    edges |= set(s.edges())
    print("a whole matrix: run bins", total.tolist(), "edge values", sorted(edges))
    assert all(total > 0)
    assert edges == set(cc.RUN_EDGES)
    qsizes = [(w // d, h // d) for w, h, d in cc.GEOMETRY]
    assert {w % cc.ETW for w, h in qsizes} >= {1, 2, 3} and any(h % cc.ETH == 1 for w, h in qsizes)   # last column tiles of 1, 2, 3 px; a last row tile of one row
    assert any(w <= cc.ETW and h <= cc.ETH for w, h in qsizes)                                        # a single emit tile
    assert any(d == 2 and (w // d) % 2 == 1 and (h // d) % 2 == 1 for w, h, d in cc.GEOMETRY)         # a decimated image of odd sides


def test_many_runs_case(oracle):
    """b: more than 8192 runs in the frame (the second round of k_scatter's loop: its 1024 or 128 waves take 8192 runs per round),
    yet no more kept clusters (9600) or pairs (32768 table entries) than a 640 x 480 handle has room for by default, nor more runs
    than its run list (4 x 9600)."""
    c = cc.MANY_RUNS
    s, _ = _stats(oracle, cc.frame("noise", c["w"], c["h"], c["seed"]), c["min_component_px"])
    print("b", s.line())
    assert s.runs > 8192
    assert s.kept <= 9600 and s.pairs <= 32768 and s.runs <= 4 * 9600
    assert int(s.pairs_per_tile.max()) <= 512


def test_deal_cases(oracle):
    """c: the 24 frames are all different and (flat ones apart) all keep clusters, so a frame that lands in another frame's place
    cannot pass; 130 x 49 is 3 x 4 emit tiles with ragged last ones."""
    fr = [cc.deal_frame(j) for j in range(24)]
    assert len({f.tobytes() for f in fr}) == 24
    keys = []
    for j, f in enumerate(fr):
        s, (th, lab, sz) = _stats(oracle, f, cc.DEAL_MIN_COMPONENT)
        print(f"c frame {j}: {s.line()}")
        assert s.kept >= 3
        keys.append(frozenset(cc.oracle_clusters(oracle, f, cc.DEAL_MIN_COMPONENT)))
    assert len(set(keys)) == 24   # no two frames even have the same cluster keys
    assert cc.DEAL_W % cc.ETW and cc.DEAL_H % cc.ETH


def test_cluster_size_gate_cases(oracle):
    """d: clusters of exactly 670, 672 and 674 points on a 64 x 48 frame whose bound is 672; 4 shapes of 20, 3 of 24 and 5 of 26
    points, one of each across an emit-tile corner, and what each min_cluster_pixels keeps of them."""
    assert cc.gate(cc.UPPER_W, cc.UPPER_H) == (24, 672)
    for pts in (670, 672, 674):
        s, _ = _stats(oracle, cc.upper_gate_frame(pts), 25)
        print(f"d upper {pts}: {s.line()} sizes {s.cluster_sizes.tolist()}")
        assert s.cluster_sizes.tolist() == [pts] and s.kept == (1 if pts <= 672 else 0)
    im = cc.lower_gate_frame()
    for mcl, kept in ((24, 3 + 5), (26, 5), (5, 3 + 5)):
        s, _ = _stats(oracle, im, 1, min_cluster_pixels=mcl)
        print(f"d lower min_cluster_pixels={mcl}: {s.line()}")
        assert sorted(s.cluster_sizes.tolist()) == [20] * 4 + [24] * 3 + [26] * 5
        assert s.kept == kept
    for pts, at in cc.LOWER_AT.items():
        x, y = at[0]
        assert (x + 1) % cc.ETW == 0 and (y + 1) % cc.ETH == 0   # the first copy has pixels in four emit tiles


def _tiles_touched(th, lab, root):
    ys, xs = np.nonzero(lab == root)
    return {(int(y) // cc.CCL_TH, int(x) // cc.CCL_TW) for y, x in zip(ys, xs)}, ys, xs


@pytest.mark.parametrize("m,w,h", cc.COMPONENT_GATE)
def test_component_size_gate_cases(oracle, m, w, h):
    """e: every region is one black component of exactly the pixel count it was built for (m - 1, m, m + 1); the m - 1 ones are in no
    cluster, the others in exactly one kept cluster each; the placements are what they claim."""
    regions = cc.component_gate_regions(m, w, h)
    im = cc.component_gate_frame(m, w, h)
    s, (th, lab, sz) = _stats(oracle, im, m)
    print(f"e m={m}: {s.line()}")
    want = cc.oracle_clusters(oracle, im, m)
    reps = {r for k in want for r in k}
    assert not np.any(th == 127)
    spans = []
    for x0, y0, rw, target in regions:
        assert th[y0, x0] == 0 and sz[y0, x0] == target, (x0, y0, int(sz[y0, x0]), target)
        root = int(lab[y0, x0])
        assert (root in reps) == (target >= m), (target, m)
        tiles, ys, xs = _tiles_touched(th, lab, root)
        interior = len(tiles) == 1 and ys.min() % cc.CCL_TH > 0 and ys.max() % cc.CCL_TH < cc.CCL_TH - 1 and xs.min() % cc.CCL_TW > 0 and xs.max() % cc.CCL_TW < cc.CCL_TW - 1
        spans.append((interior, len({t[0] for t in tiles}), len({t[1] for t in tiles})))
    print(f"e m={m}: (interior, tile rows, tile columns) per region {spans}")
    assert len(want) == sum(1 for r in regions if r[3] >= m) == s.kept
    if m in (25, 1000):
        assert [sp[0] for sp in spans] == [True] * 3 + [False] * 6          # inside one tile, off its ring
        assert all(sp[1] == 2 and sp[2] == 2 for sp in spans[3:6])          # across a tile corner
        assert all(sp[1] == (3 if m == 1000 else 2) for sp in spans[6:9])   # down a column of tiles
    else:
        assert all(sp[1] > 2 and sp[2] >= 2 for sp in spans)


def test_table_limit_cases(oracle):
    """f: one emit tile of the 512-pair frame holds exactly 512 distinct pairs, one of the 552-pair frame 552 (of 888 in the frame);
    neither frame keeps a cluster, and neither comes near the handle's capacities (1700 clusters, 4096 table entries, 6800 runs)."""
    for pairs, frame_pairs in ((512, 512), (552, 888)):
        s, _ = _stats(oracle, cc.table_frame(pairs), 1)
        print(f"f {pairs}: {s.line()}")
        assert int(s.pairs_per_tile.max()) == pairs and s.pairs == frame_pairs and s.kept == 0
        assert s.pairs <= 1700 and s.runs <= 4 * 1700
    for f in cc.table_tag_frames():
        s, _ = _stats(oracle, f, 1)
        print(f"f tags: {s.line()}")
        assert s.kept >= 10 and int(s.pairs_per_tile.max()) <= 512 and s.pairs <= 1700 and s.runs <= 4 * 1700


def test_dotted_region_needs_its_dots(oracle):
    """Without the dots a region's flat interior thresholds to 127 and the component is a rim; with them it is whole."""
    w, h = 256, 128
    im = cc.dotted_region(w, h, [(20, 20, 100, 5000)])
    th, lab, sz = cc.oracle_stages(oracle, im)
    assert sz[20, 20] == 5000 and not np.any(th == 127)
    plain = cc.dotted_region(w, h, [(20, 20, 100, 5000)], dark_dot=215, light_dot=40)   # the dots in the colour of their surroundings
    th2, lab2, sz2 = cc.oracle_stages(oracle, plain)
    assert np.any(th2 == 127) and sz2[20, 20] < 5000
