"""GPU: the count pass of k_emit2 reads its leaders from the row table (k_clusters.hip, ck_emit_row.h).  Point-for-point parity of
clusters() with the CPU oracle on small frames that put every kind of pixel row at every place the kernel treats differently
(tests/emit_row_cases.py; tests/test_emit_row_host.py shows with the oracle alone which kinds and places the frames reach): 66 x 17,
67 x 18, 129 x 33 and 130 x 35 — an emit-tile seam in x and in y, ragged last columns and rows, widths that are no multiple of 4 —
at min_component_px 5 and 25, with twins merged and not (CK_EMIT_TWINS=0), plain and on poisoned buffers."""
import os
import subprocess
import sys

import pytest

import cluster_cases as cc
import emit_row_cases as ec
from emit_rows_child import check_batch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N_FRAMES = sum(len(ec.frames(w, h)) for w, h in ec.SIZES) * len(ec.MIN_COMPONENT) + len(ec.rim_noise()[3])


@pytest.mark.parametrize("mcp", ec.MIN_COMPONENT)
@pytest.mark.parametrize("w,h", ec.SIZES)
def test_every_row_kind_at_every_place(oracle, w, h, mcp):
    """Stairs both ways, stripes of 1, 2 and 3 pixels both ways, checkers of 3 and 5, blobs at three densities and the lattices whose
    dark component meets four light ones at every crossing: one call per size and gate on the product library."""
    assert check_batch(oracle, w, h, mcp, ec.frames(w, h)) > 0


def test_three_leaders_at_the_last_emitting_column(oracle):
    """Noise at min_component_px = 1: the one-pixel components of column w - 1 give rows of three leaders in column w - 2."""
    w, h, mcp, named = ec.rim_noise()
    assert check_batch(oracle, w, h, mcp, named) > 0


def _child(**knobs):
    from conftest import diag_env
    r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.join(HERE, "emit_rows_child.py")], capture_output=True, text=True,
                       env=diag_env(**knobs), timeout=180)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("EMIT_ROWS_CHILD ")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return [int(v) for v in lines[0].split()[1:]]


@pytest.mark.parametrize("knobs", [dict(CK_POISON="1"), dict(CK_EMIT_TWINS="0"), dict(CK_EMIT_TWINS="0", CK_POISON="1")],
                         ids=["poisoned", "twins off", "twins off, poisoned"])
def test_the_same_frames_on_the_diagnostics_build(oracle, knobs):
    """Every frame above in a child process on the diagnostics build (its knobs are read once per process): buffers that start as 0xA5
    bytes, every point stored on its own (the table's entries are the same, the absorb / drop bits never set), and both.  The child
    checks every frame against the oracle; the number of points returned does not depend on how they are stored."""
    frames, points = _child(**knobs)
    assert frames == N_FRAMES and points > 0
