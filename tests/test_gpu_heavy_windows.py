"""The split quad fit's middle kernel (k_chunk) on the heaviest windows a frame can hold: full-contrast edges along an axis, at 45
degrees and at a shallow angle (tests/heavy_window_cases.py), quad for quad against the oracle, equality of bytes after the (rep0,
rep1) sort.  k_chunk takes 1 / W of a window from a table indexed by the window's weight sum, without a branch, and forms its
running sums across the four waves of a workgroup from the waves' totals; each frame is placed (CK_EXT_BASE, the diagnostics
build) so that the middle of its heaviest window — 41 points of weight 361 in the diagonal frame, the top of the table's range —
lies on each of the three wave boundaries of the loaded span and on the first position of a span.  The conditions on the frames are
asserted on the CPU before the device is asked for anything (the fixture; tests/test_heavy_window_cases_host.py has them without
a GPU).

Each run is a child process (tests/span_alignment_child.py) on the diagnostics build with CK_FIT_FLAT=2, plain and on poisoned
buffers, under a time limit of its own; after a child that did not end by itself nothing more is started.

Measured on an MI355X, the whole child process (interpreter start, three handles, 36 calls): 0.48 s plain, 0.41 s poisoned (the
calls themselves 0.02 s).  On a mutant of the diagnostics library (never committed) that sums the waves in front of a wave from one
wave too few, both cases fail, as do all of tests/test_gpu_span_alignment.py, test_gpu_tail_prefix.py and test_gpu_tail_selection.py."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import heavy_window_cases as hw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# seconds a child may take: five times its measured run time (0.48 s at most, above), as in tests/test_gpu_span_alignment.py,
# because the machine is shared
LIMIT = 3


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    fig, quads = hw.check(oracle)
    data = {}
    for (name, _, _, _), f, q in zip(hw.CASES, hw.frames(), quads):
        data["f_" + name] = f[None]
        data["q_%s_0" % name] = q
    path = str(tmp_path_factory.mktemp("heavy_windows") / "cases.npz")
    np.savez(path, **data)
    return path, fig


_ended_badly = []


@pytest.mark.parametrize("poison", [False, True])
def test_heaviest_window_on_every_wave_and_span_boundary(cases, poison):
    """One child: every frame at its own four bases and at the other frames' (twelve bases, three handles, 36 calls)."""
    assert not _ended_badly, "an earlier child did not end by itself: nothing more is started on the device: %s" % _ended_badly
    from conftest import diag_env
    path, fig = cases
    names = [c[0] for c in hw.CASES]
    bases = sorted(set(b for n in names for b in hw.bases(fig[n][5])))
    assert len(bases) == 12
    env = diag_env(CK_FIT_FLAT="2", **({"CK_POISON": "1"} if poison else {}))
    env.pop("CK_EXT_BASE", None)
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.join(HERE, "span_alignment_child.py"), path, ",".join(names),
                        ",".join(str(b) for b in bases)], capture_output=True, text=True, env=env, timeout=LIMIT + 60)
    if r.returncode not in (0, 1):
        _ended_badly.append((poison, r.returncode))
    out = {ln.split()[0]: ln.split()[1] for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("CALLS", "MISMATCHES", "HASH", "SECONDS")}
    assert len(out) == 4, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(bases, poison, out, "child's run time %.2f s of %d" % (time.time() - t0, LIMIT))
    assert int(out["CALLS"]) == 3 * 12
    assert int(out["MISMATCHES"]) == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
