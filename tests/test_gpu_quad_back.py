"""The back half of the quad fit (smoothing window, local maxima, the cut to max_nmaxima, line fits, the 4-subset search and its
tie-break, the corner, area, angle and winding checks, edge refinement) at its own edges, quad for quad, in both forms of the fit: k_fit
and the batch plan (the product library, in this process) and k_seq -> k_chunk -> k_tail (the split fit, forced for every call by
CK_FIT_FLAT=2 on the diagnostics build, in a child process: tests/quad_back_child.py, once plain and once on poisoned buffers).
Equality of bytes against the oracle; the cases are tests/quad_cases.py's, and the conditions they have to meet are asserted on the
oracle's per-cluster readout, on the CPU, before the device is asked for anything."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import quad_cases as qc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """Every case traced once on the oracle, its conditions asserted (qc.measure), frames, settings and expected quads in one .npz."""
    data, figures = {}, {}
    for name in qc.NAMES:
        frames, settings, _ = qc.case(name)
        figures[name], quads, index, _ = qc.measure(oracle, name)
        data["f_" + name], data["u_" + name], data["s_" + name] = frames, np.asarray(index), np.asarray(json.dumps(settings))
        for i, q in quads.items():
            data["q_%s_%d" % (name, i)] = q
    path = str(tmp_path_factory.mktemp("quad_back") / "cases.npz")
    np.savez(path, **data)
    return path, data, figures


@pytest.mark.parametrize("name", qc.NAMES)
def test_back_half_on_the_product_library(cases, name):
    """In this process: a call of a few frames runs k_fit, its size classes side by side; the 40 frames of batch_* and the 17 / 33 of
    classes_* take the batch plan, which has k_fit's 128-thread class too."""
    from quad_back_child import run_case
    _, data, figures = cases
    assert name in figures   # (the conditions held: the fixture asserts them)
    bad = run_case(data, name)
    assert not bad, f"{name}: frames that differ from the oracle (frame, device quads, oracle quads): {bad}"


def _child(path, **knobs):
    """The cases in a child process on the diagnostics build with the split fit forced; its GPU work runs under a time limit of its own."""
    from conftest import diag_env
    env = diag_env(CK_FIT_FLAT="2", **knobs)   # (knobs of the diagnostics build)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "quad_back_child.py"), path], capture_output=True,
                       text=True, env=env, timeout=300)
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


def test_back_half_in_the_split_fit(cases, child_runs):
    bad, _, r = child_runs[0]
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_back_half_in_the_split_fit_on_poisoned_buffers(cases, child_runs):
    """An entry read without having been written would show as a quad that differs."""
    assert child_runs[1] is not child_runs[0], "the plain run did not end by itself"
    bad, _, r = child_runs[1]
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_split_fit_is_deterministic(child_runs):
    """The same calls in a second process, on buffers that start differently: identical quads."""
    assert child_runs[1] is not child_runs[0] and child_runs[0][1] == child_runs[1][1]
