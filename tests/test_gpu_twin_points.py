"""GPU: diagonal twin points (k_clusters.hip: k_emit2 stores the two points a straight edge emits at one half-pixel as one word;
k_scan counts them twice for the size gates and the overflow bits, once for the offsets) must not show in anything the library
returns: clusters point for point and detections and status bit for bit what the CPU oracle returns, on hand-drawn frames that
put the twins where the merge could go wrong (tests/twin_cases.py; tests/test_twin_points_host.py shows with the oracle alone that
the frames reach those places)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases as cc
import twin_cases as tc
from chalkydri_amd import _abi as A
from chalkydri_amd import default_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FULL = A.CK_FRAME_POINTS_OVERFLOW | A.CK_FRAME_CLUSTERS_OVERFLOW
# Cluster records for every frame here, counted either way: the oracle counts every component pair towards max_clusters_per_frame,
# the device only those inside the size gates (the 2 x 2 checkerboard at min_component_px = 1 has 1 944 pairs, none of them kept, and
# the default of 1 024 records).  These tests are about the points.
CLUSTER_ROOM = 8192


def _detector(*a, **kw):
    from chalkydri_amd.detector import AprilTagDetector
    return AprilTagDetector(*a, **kw)


def _same_dets(have, want):
    assert len(have) == len(want), f"{len(have)} vs {len(want)} detections"
    for a, b in zip(have, want):
        assert (a.id(), a.hamming(), a.family()) == (b["id"], b["hamming"], b["family"])
        assert np.float32(a.decision_margin()) == np.float32(b["margin"])
        assert np.array_equal(a.center(), b["c"]) and np.array_equal(a.corners(), b["p"])


def _check(oracle, frames, names, tag, **settings):
    """clusters() and detect_batch() of the frames on one handle with `settings` against the oracle with the same settings"""
    n, (h, w) = len(frames), frames[0].shape
    settings.setdefault("max_clusters_per_frame", CLUSTER_ROOM)
    mcp, mcl = settings.get("min_component_px", 25), settings.get("min_cluster_pixels", 24)
    wants = [cc.oracle_clusters(oracle, f, mcp, mcl) for f in frames]
    det = _detector(w, h, max_batch=n, **settings)
    ccap, pcap = cc.caps_for(wants)
    got = det.clusters(np.stack(frames), cluster_cap=ccap, point_cap=pcap)
    for i in range(n):
        cc.check_frame(got[i], wants[i], f"{tag} {names[i]}")
    dets, status = det.detect_batch(np.stack(frames), cap=64, return_status=True)
    cfg = default_config(w, h, **settings)
    for i in range(n):
        want, st = oracle.detect(frames[i], cfg)
        assert status[i] == st, f"{tag} {names[i]}: status {status[i]} vs {st}"
        _same_dets(dets[i], want)
    det.close()
    return wants


@pytest.mark.parametrize("mcp", tc.EDGE_MIN_COMPONENT)
def test_edges_at_tile_boundaries_frame_rim_and_mixed_clusters(oracle, mcp):
    """Straight edges across the emit-tile boundaries x = 63|64 and y = 15|16 (the absorbing and the dropping thread sit in
    different workgroups), edges through columns 1 and w - 2 and rows 1 and h - 2 and one further out (one copy has no emitting
    owner: nothing may merge), checkerboards of 2 x 2 and 3 x 3 cells (twins of different clusters side by side) and a 45 degree
    staircase (no twins): one batch, at min_component_px 25 and 1."""
    frames = tc.edge_frames()
    _check(oracle, list(frames.values()), list(frames), f"min_component_px={mcp}", min_component_px=mcp)


@pytest.mark.parametrize("gate", sorted(tc.GATES))
def test_size_gate_counts_twins_twice(oracle, gate):
    """A cluster of exactly min_cluster_pixels points is kept, one of a point fewer is dropped, at min_cluster_pixels 24 and 50 —
    both have fewer stored words than that (17 and 19, 37 and 35 distinct coordinates), so a gate on the stored count would drop
    both, and the kept one reaches the fit below its own floor of 24 / has to pass it on the stored count."""
    f = tc.gate_frame(gate)
    wants = _check(oracle, [f], [f"gate {gate}"], "gate", min_component_px=1, min_cluster_pixels=gate)
    assert [len(v) for v in wants[0].values()] == [tc.GATES[gate][1]]


def test_point_capacity_between_stored_and_counted_points(oracle):
    """max_points_per_frame = the frame's points counted as the oracle counts them: no overflow bit; one less, and half way down to
    the number of stored words (where every word still fits): the points-or-clusters overflow is reported as the oracle reports
    it.  Frames with and without twins in one batch."""
    frames = tc.edge_frames()
    names = ["tile cross", "mixed checker3", "mixed staircase"]
    batch = np.stack([frames[k] for k in names])
    for name in names:
        logical, physical = tc.totals(oracle, frames[name], 1)
        for cap in sorted({logical, logical - 1, (logical + physical) // 2}):
            settings = dict(min_component_px=1, max_points_per_frame=cap, max_clusters_per_frame=CLUSTER_ROOM)
            det = _detector(tc.W, tc.H, max_batch=len(names), **settings)
            cfg = default_config(tc.W, tc.H, **settings)
            dets, status = det.detect_batch(batch, cap=64, return_status=True)
            for i, other in enumerate(names):
                want, st = oracle.detect(frames[other], cfg)
                assert bool(status[i] & FULL) == bool(st & FULL), f"cap {cap} ({name}: {physical} stored, {logical} counted), frame {other}"
                if other == name:
                    assert bool(st & FULL) == (cap < logical)
                if not (st & FULL):   # (which clusters survive a full buffer is not part of the contract; that it is reported is)
                    assert status[i] == st
                    _same_dets(dets[i], want)
            det.close()


def _child(twins):
    from conftest import diag_env
    env = diag_env(CK_EMIT_TWINS=str(twins))   # (a knob of the diagnostics build, read once per process: hence the child)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(HERE, "twin_points_child.py")], capture_output=True, text=True,
                       env=env, timeout=150)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("TWIN_CHILD ")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return lines[0].split()[1:]


def test_merge_switched_off_returns_the_same(oracle):
    """The diagnostics build with CK_EMIT_TWINS=0 (every point stored on its own) and =1 (the product's behaviour): identical
    clusters() and detections on two random 320 x 200 frames, and both equal to the oracle's (the child compares)."""
    off, on = _child(0), _child(1)
    assert off == on and int(on[0]) > 0 and int(on[1]) == 0, (off, on)
