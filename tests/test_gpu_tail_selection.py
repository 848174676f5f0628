"""The rank selection of the quad fit's last kernel (k_tail, 5a: the cut of a cluster's maxima to the max_nmaxima strongest) at the sizes
where it changes its way — 64 | 65 maxima, 64 RV | 64 RV + 1, well beyond —, with a tie across the cut and a cluster in three or more
spans on the register path, under max_nmaxima 4, 10 and 12: quad for quad against the oracle, equality of bytes.  The cases are
tests/tail_selection_cases.py's, their conditions asserted on the oracle's readout, on the CPU, before the device is asked for anything;
they run through tests/quad_back_child.py in a child process on the diagnostics build with the split fit forced for every call
(CK_FIT_FLAT=2), once plain and once on poisoned buffers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tail_selection_cases as tc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """Every case traced once on the oracle, its conditions asserted (tc.measure); frames, settings and expected quads in one .npz."""
    data, figures = {}, {}
    for name in tc.NAMES:
        frames, settings, _ = tc.case(name)
        figures[name], quads, index, _ = tc.measure(oracle, name)
        data["f_" + name], data["u_" + name], data["s_" + name] = frames, np.asarray(index), np.asarray(json.dumps(settings))
        for i, q in quads.items():
            data["q_%s_%d" % (name, i)] = q
    path = str(tmp_path_factory.mktemp("tail_selection") / "cases.npz")
    np.savez(path, **data)
    return path, figures


def _child(path, **knobs):
    """The cases in a child process on the diagnostics build with the split fit forced; its GPU work runs under a time limit of its own."""
    from conftest import diag_env
    env = diag_env(CK_FIT_FLAT="2", **knobs)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(HERE, "quad_back_child.py"), path], capture_output=True,
                       text=True, env=env, timeout=180)
    lines = r.stdout.splitlines()
    bad = [ln for ln in lines if ln.startswith("MISMATCHING_CASES")]
    hashes = [ln for ln in lines if ln.startswith("HASH")]
    assert bad and hashes, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return int(bad[0].split()[1]), hashes[0].split()[1], r


@pytest.fixture(scope="module")
def child_runs(cases):
    """two runs of the child on the same file: plain, and with the handles' buffers starting as 0xA5 bytes"""
    plain = _child(cases[0])
    if plain[2].returncode not in (0, 1):   # (ended by a signal or its time limit: nothing more is started on the device)
        return [plain, plain]
    return [plain, _child(cases[0], CK_POISON="1")]


def test_selection_in_the_split_fit(cases, child_runs):
    assert set(cases[1]) == set(tc.NAMES)   # (the conditions held: the fixture asserts them)
    bad, _, r = child_runs[0]
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_selection_in_the_split_fit_on_poisoned_buffers(child_runs):
    """A maximum read without having been written would show as a quad that differs."""
    assert child_runs[1] is not child_runs[0], "the plain run did not end by itself"
    bad, _, r = child_runs[1]
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_selection_is_deterministic(child_runs):
    """The same calls in a second process, on buffers that start differently: identical quads."""
    assert child_runs[1] is not child_runs[0] and child_runs[0][1] == child_runs[1][1]
