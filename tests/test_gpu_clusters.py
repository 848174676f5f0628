"""GPU parity of the gradient-cluster stage (k_clusters.hip: k_clear, k_emit2, k_scan, k_scatter) at the stage's own edges, point for
point and bit for bit against the CPU oracle.  Every cluster the oracle has inside k_scan's gates must come back under the same key
with the same points (as sorted sets: the order inside a cluster is not defined on the device), and the records' start / count must
tile the point array.  The inputs are built in tests/cluster_cases.py; tests/test_cluster_cases_host.py shows, with the oracle
alone, that each of them reaches the edge it is named for (runs per frame, run lengths, pairs per emit tile, exact sizes)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases as cc
from chalkydri_amd import _abi as A
from chalkydri_amd import default_config

pytestmark = pytest.mark.gpu


def _detector(*a, **kw):
    from chalkydri_amd.detector import AprilTagDetector
    return AprilTagDetector(*a, **kw)


def _compare(det, frames, wants, tag):
    ccap, pcap = cc.caps_for(wants)
    got = det.clusters(frames, cluster_cap=ccap, point_cap=pcap)
    assert len(got) == len(wants)
    for i, want in enumerate(wants):
        cc.check_frame(got[i], want, f"{tag} frame {i}")
    return got


def _sorted_bytes(got):
    """A call's result without what the device leaves undefined (the order of clusters and of a cluster's points)."""
    out = []
    for cl, pts in got:
        d = cc.cluster_dict(cl, pts)
        out.append(b"".join(np.asarray(k, np.int64).tobytes() + d[k].tobytes() for k in sorted(d)))
    return out


# ---- a. geometry x content x gate ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mcp", cc.GEOMETRY_MIN_COMPONENT)
@pytest.mark.parametrize("w,h,dec", cc.GEOMETRY)
def test_geometry_content_gate(oracle, w, h, dec, mcp):
    """Ragged emit tiles (a last column tile of 1, 2 or 3 pixels, a last row tile of one row, a single tile, decimated images of odd
    sides) under noise, blobs, stripes, spiral and rendered tags, three frames of different seeds on a handle of four, at
    min_component_px 25 and 5.  Over this matrix the kept clusters' (tile, pair) runs fall into every class of k_scatter (1..16,
    17..64, 65..256, >= 257 points) and runs of exactly 16, 17, 64, 65, 256 and 257 points all occur in it — found in the seeded
    frames themselves (640 x 480 noise, seed 3, has all six on its own), so no comb frame had to be added for them."""
    det = _detector(w, h, max_batch=4, quad_decimate=dec, min_component_px=mcp)
    for kind in cc.geometry_kinds(w, h, dec):
        frames = cc.geometry_frames(w, h, kind)
        wants = [cc.oracle_clusters(oracle, f, mcp, dec=dec) for f in frames]
        _compare(det, frames, wants, f"{w}x{h}/{dec} {kind} min_component_px={mcp}")
    det.close()


# ---- b. many runs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
def test_many_runs(oracle, n):
    """More than 8192 (tile, pair) runs in one frame: the second round of k_scatter's loop over the run list, in the variant for calls
    of up to four frames (n = 1) and in the batch variant (the frame in the middle of n = 5).  640 x 480 noise at min_component_px = 1:
    26 314 runs, 21 693 pairs, 5 415 kept clusters (oracle)."""
    c = cc.MANY_RUNS
    busy = cc.frame("noise", c["w"], c["h"], c["seed"])
    frames = np.stack([busy] if n == 1 else [cc.frame("blobs", c["w"], c["h"], 5), cc.frame("stripes", c["w"], c["h"], 0), busy,
                                             cc.frame("tags", c["w"], c["h"], 6), cc.frame("spiral", c["w"], c["h"], 0)])
    wants = [cc.oracle_clusters(oracle, f, c["min_component_px"]) for f in frames]
    det = _detector(c["w"], c["h"], max_batch=n, min_component_px=c["min_component_px"])
    _compare(det, frames, wants, f"many runs n={n}")
    det.close()


# ---- c. batch dealing -----------------------------------------------------------------------------------------------------------------
_deal = {}


def _deal_case(oracle, j):
    if j not in _deal:
        f = cc.deal_frame(j)
        _deal[j] = (f, cc.oracle_clusters(oracle, f, cc.DEAL_MIN_COMPONENT))
    return _deal[j]


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("n", cc.DEAL_N)
def test_batch_dealing(oracle, n, extra):
    """Calls of 16 frames and more deal their frames to the XCDs (frame = (j / tiles) * 8 + x, workgroups past the last frame return
    at once); smaller ones do not.  n either side of 16, multiples of 8 and not, on handles of exactly n and of n + 3 frames; every
    frame is different, and every one must come back as itself."""
    cases = [_deal_case(oracle, j) for j in range(n)]
    det = _detector(cc.DEAL_W, cc.DEAL_H, max_batch=n + extra, min_component_px=cc.DEAL_MIN_COMPONENT)
    _compare(det, np.stack([c[0] for c in cases]), [c[1] for c in cases], f"dealing n={n} max_batch={n + extra}")
    det.close()


def test_calls_of_changing_size_on_one_handle(oracle):
    """24 noise frames, 2 flat ones, 17 of blobs, the 24 again on one handle: the second and third calls leave the first one's run
    records and fill cursors under theirs, the fourth meets the third's.  Every result equals the oracle's, and the first and the
    last call return the same bytes."""
    w, h, mcp = cc.DEAL_W, cc.DEAL_H, cc.DEAL_MIN_COMPONENT
    calls = [cc.frames("noise", w, h, 24, 31), cc.frames("flat", w, h, 2, 32), cc.frames("blobs", w, h, 17, 33)]
    calls.append(calls[0])
    wants = [[cc.oracle_clusters(oracle, f, mcp) for f in fr] for fr in calls[:3]]
    wants.append(wants[0])
    assert all(len(x) == 0 for x in wants[1]) and all(len(x) >= 3 for x in wants[0] + wants[2])
    det = _detector(w, h, max_batch=24, min_component_px=mcp)
    got = [_compare(det, fr, wa, f"call {k}") for k, (fr, wa) in enumerate(zip(calls, wants))]
    assert _sorted_bytes(got[0]) == _sorted_bytes(got[3])
    det.close()


# ---- d. cluster-size gates ------------------------------------------------------------------------------------------------------------
def test_largest_cluster_kept(oracle):
    """k_scan keeps count <= 3 * (2 w + 2 h) = 672 on a 64 x 48 frame: combs whose outline is a cluster of exactly 670, 672 and 674 points
    — the first two come back, the third does not."""
    sizes = (670, 672, 674)
    frames = np.stack([cc.upper_gate_frame(p) for p in sizes])
    wants = [cc.oracle_clusters(oracle, f) for f in frames]
    assert [[len(v) for v in w.values()] for w in wants] == [[670], [672], []]
    det = _detector(cc.UPPER_W, cc.UPPER_H, max_batch=3)
    got = _compare(det, frames, wants, "upper gate")
    assert [[int(c) for c in cl[:, 3]] for cl, _ in got] == [[670], [672], []]
    det.close()


@pytest.mark.parametrize("min_cluster_pixels,kept", [(24, [24] * 3 + [26] * 5), (26, [26] * 5), (5, [24] * 3 + [26] * 5)])
def test_smallest_cluster_kept(oracle, min_cluster_pixels, kept):
    """k_scan keeps count >= max(24, min_cluster_pixels): shapes of exactly 20, 24 and 26 points (min_component_px = 1), several of each,
    one of each across an emit-tile corner (its points come from four tiles' runs).  A min_cluster_pixels below 24 does not lower
    the floor of 24."""
    im = cc.lower_gate_frame()
    want = cc.oracle_clusters(oracle, im, 1, min_cluster_pixels)
    assert sorted(len(v) for v in want.values()) == kept
    det = _detector(cc.LOWER_W, cc.LOWER_H, max_batch=1, min_component_px=1, min_cluster_pixels=min_cluster_pixels)
    got = _compare(det, im[None], [want], f"lower gate {min_cluster_pixels}")
    assert sorted(int(c) for c in got[0][0][:, 3]) == kept
    det.close()


# ---- e. component-size gate -----------------------------------------------------------------------------------------------------------
def _component_gate_case(oracle, m, w, h):
    im = cc.component_gate_frame(m, w, h)
    want = cc.oracle_clusters(oracle, im, m)
    assert len(want) == 2 * len(cc.component_gate_regions(m, w, h)) // 3   # the regions of m and m + 1 pixels, not those of m - 1
    return im, want


@pytest.mark.parametrize("m,w,h", cc.COMPONENT_GATE)
def test_component_size_gate(oracle, m, w, h):
    """min_component_px = m against black components of exactly m - 1, m and m + 1 pixels (inside one segmentation tile: the
    CK_LBL_SMALL flag; across tiles: the size tables of k_fmerge, 16-bit saturating up to 0x7FFF, in global memory above): the
    m - 1 regions give no cluster, the others one each.  0x8000, 40000 and 70000 are past what the 16-bit sizes express."""
    im, want = _component_gate_case(oracle, m, w, h)
    det = _detector(w, h, max_batch=1, min_component_px=m)
    _compare(det, im[None], [want], f"component gate m={m}")
    det.close()


def component_gate_merge_paths():
    """Runs in a child process against the diagnostics build (the knobs do not exist in the product library)."""
    import pyoracle
    from chalkydri_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"CK_FMERGE_CAP" in blob and b"CK_FMERGE_BAND_ROWS" in blob, "not the diagnostics build: " + _lib.LIB_PATH
    runs = 0
    for m, w, h in cc.COMPONENT_GATE:
        im, want = _component_gate_case(pyoracle, m, w, h)
        det = _detector(w, h, max_batch=1, min_component_px=m)
        for cap in (64, 2000):
            for rows in (0, 1, 3):
                os.environ["CK_FMERGE_CAP"] = str(cap)   # (both read per call)
                os.environ["CK_FMERGE_BAND_ROWS"] = str(rows)
                _compare(det, im[None], [want], f"component gate m={m} CK_FMERGE_CAP={cap} CK_FMERGE_BAND_ROWS={rows}")
                runs += 1
        det.close()
    print("COMPONENT_GATE_OK", runs)


def test_component_size_gate_on_every_merge_path(oracle):
    """The same frames with the merge kernel's paths forced (CK_FMERGE_CAP 64: global memory, 2000: LDS; CK_FMERGE_BAND_ROWS 1 and 3:
    frames joined in bands of tile rows, whose seams add sizes saturating) — knobs of the diagnostics build, hence the child."""
    from conftest import ROOT, diag_env
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import importlib.util as u; "
            "sp = u.spec_from_file_location('tcl', %r); m = u.module_from_spec(sp); sp.loader.exec_module(m); m.component_gate_merge_paths()"
            % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=diag_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "COMPONENT_GATE_OK 36" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- f. the 512 entries of k_emit2's LDS table ---------------------------------------------------------------------------------------
def _table_batch(oracle, pairs):
    tags = cc.table_tag_frames()
    frames = np.stack([tags[0], cc.table_frame(pairs), tags[1]])
    cfg = default_config(cc.TABLE_W, cc.TABLE_H, min_component_px=1)
    wants = [cc.oracle_clusters(oracle, f, 1) for f in frames]
    dets = [oracle.detect(f, cfg) for f in frames]
    assert len(wants[1]) == 0 and all(len(d[0]) >= 1 for d in (dets[0], dets[2])) and not dets[1][1]
    return frames, wants, dets


def _check_dets(got, status, dets, frames_idx):
    from test_gpu_detect import _same_dets
    for i in frames_idx:
        assert status[i] == dets[i][1], f"status of frame {i}: {status[i]} vs the oracle's {dets[i][1]}"
        _same_dets(got[i], dets[i][0])


def test_emit_table_exactly_full(oracle):
    """512 distinct component pairs inside one 64 x 16 emit tile (a one-pixel checkerboard over exactly that tile, min_component_px = 1)
    fill the tile's table to its last entry: nothing is dropped, no status bit is raised — clusters, detections and status of
    the frame and of its batch neighbours equal the oracle's."""
    frames, wants, dets = _table_batch(oracle, 512)
    det = _detector(cc.TABLE_W, cc.TABLE_H, max_batch=3, min_component_px=1)
    _compare(det, frames, wants, "table full")
    got, status = det.detect_batch(frames, cap=64, return_status=True)
    _check_dets(got, status, dets, (0, 1, 2))
    det.close()


def test_emit_table_overflow_is_a_status_bit(oracle):
    """552 distinct pairs inside one emit tile are more than its table holds.  The documented limit (include/chalkydri_hip.h at
    CK_FRAME_CLUSTERS_OVERFLOW): the frame's CK_FRAME_CLUSTERS_OVERFLOW bit is set, which the oracle does not do; the
    call returns; the frame's batch neighbours are untouched (clusters, detections and status equal the oracle's); and the next call
    on the handle is clean."""
    frames, wants, dets = _table_batch(oracle, 552)
    det = _detector(cc.TABLE_W, cc.TABLE_H, max_batch=3, min_component_px=1)
    ccap, pcap = cc.caps_for(wants)
    cl = det.clusters(frames, cluster_cap=ccap, point_cap=pcap)
    for i in (0, 2):
        cc.check_frame(cl[i], wants[i], f"table overflow, neighbour {i}")
    got, status = det.detect_batch(frames, cap=64, return_status=True)
    assert status[1] & A.CK_FRAME_CLUSTERS_OVERFLOW and dets[1][1] == 0
    assert not status[1] & ~A.CK_FRAME_CLUSTERS_OVERFLOW and len(got[1]) == 0
    _check_dets(got, status, dets, (0, 2))
    # the next call on the handle: the exactly-full frame between the same neighbours, clean
    frames2, wants2, dets2 = _table_batch(oracle, 512)
    _compare(det, frames2, wants2, "after the overflow")
    got2, status2 = det.detect_batch(frames2, cap=64, return_status=True)
    _check_dets(got2, status2, dets2, (0, 1, 2))
    det.close()
