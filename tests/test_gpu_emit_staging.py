"""GPU: k_emit2 stages its tile in aligned groups of four pixels when the frame's width is a multiple of four (k_clusters.hip,
ck_emit_stage.h; tests/test_emit_stage_host.py checks the index arithmetic on the host).  Point-for-point parity of clusters() with
the CPU oracle on the frames of tests/emit_row_cases.py at the sizes of tests/emit_staging_cases.py — one group of a tile column inside
the frame, halo columns and rows wholly outside it, halos in another CCL tile than the groups, groups either side of the CCL seam —
at min_component_px 5 and 25; on the product library, and in child processes on the diagnostics build: poisoned buffers, the
per-pixel staging forced (CK_EMIT_STAGE4=0), both, and the per-pixel staging with every point stored on its own.
Every call fills its handle's max_batch, so the group loads read the last frame of the buffers."""
import os
import subprocess
import sys

import pytest

import emit_row_cases as ec
import emit_staging_cases as sc
from emit_rows_child import check_batch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N_FRAMES = sum(len(ec.frames(w, h)) for w, h in sc.SIZES) * len(sc.MIN_COMPONENT)


@pytest.mark.parametrize("mcp", sc.MIN_COMPONENT)
@pytest.mark.parametrize("w,h", sc.SIZES)
def test_group_staging_at_its_edges(oracle, w, h, mcp):
    """one call per size and gate on the product library: every frame at once, the handle's last frame among them"""
    assert check_batch(oracle, w, h, mcp, ec.frames(w, h)) > 0


def test_last_frame_of_a_short_batch(oracle):
    """Three frames in a handle of three (frames dealt to workgroups in order, not to XCDs as in batches of 16 and more): the group
    loads of the last one end where the threshold and label buffers end."""
    w, h = 132, 35
    named = dict(list(ec.frames(w, h).items())[-3:])
    assert check_batch(oracle, w, h, 5, named) > 0


def _child(**knobs):
    from conftest import diag_env
    r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.join(HERE, "emit_staging_child.py")], capture_output=True, text=True,
                       env=diag_env(**knobs), timeout=180)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("EMIT_STAGING_CHILD ")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return [int(v) for v in lines[0].split()[1:]]


@pytest.mark.parametrize("knobs", [dict(CK_POISON="1"), dict(CK_EMIT_STAGE4="0"), dict(CK_EMIT_STAGE4="0", CK_POISON="1"),
                                   dict(CK_EMIT_STAGE4="0", CK_EMIT_TWINS="0")],
                         ids=["poisoned", "per pixel", "per pixel, poisoned", "per pixel, twins off"])
def test_the_same_frames_on_the_diagnostics_build(oracle, knobs):
    """Every frame above in a child process on the diagnostics build (its knobs are read once per process).  The child checks every
    frame against the oracle; the number of points returned does not depend on how the tile was staged or the points stored."""
    frames, points = _child(**knobs)
    assert frames == N_FRAMES and points > 0
