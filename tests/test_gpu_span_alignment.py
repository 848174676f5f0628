"""The split quad fit's middle and last kernel (k_chunk, k_tail) at every alignment of a cluster to their grid of spans of 960, words
of 64 and blocks of 32 positions, and k_chunk's loop over several spans per workgroup: quad for quad against the oracle, equality of
bytes after the (rep0, rep1) sort.  Where a cluster lands normally follows an atomic counter; the diagnostics build's CK_EXT_BASE sets
the first position handed out in every frame of a call, and the sweep frames of tests/span_cases.py hold one cluster each, so base b
puts that cluster's points at [b + 25, b + 25 + sz).  The conditions on the inputs are asserted on the oracle's readout, on the CPU,
before the device is asked for anything (the fixture; tests/test_span_cases_host.py has them without a GPU).

Every case is a child process (tests/span_alignment_child.py) on the diagnostics build with CK_FIT_FLAT=2, under a time limit of its
own; after a child that did not end by itself nothing more is started.  The sweep: every base of 0 .. 1023 in four children of 256
bases, each base one call on the 352 handle (14 frames) and one on the 448 handle; the same on poisoned buffers at the bases around
span 0's start and the first span boundary; the crowded 640x480 frames with 8 k_chunk workgroups per frame (CK_CHUNK_WGS=0: 16 or 17
spans each), plain and poisoned, in any order of placement; the first sweep child again in a second process, hash for hash.

Measured on an MI355X, the whole child process (interpreter start, two handles, the calls): a sweep child of 512 calls 0.68 .. 0.87 s
(the calls themselves 0.28 s), a crowded child 0.43 .. 0.55 s; the two children of tests/test_gpu_tail_selection.py with their oracle traces, on the
same machine in the same run, 1.13 s together.  On two mutants of the diagnostics library (never committed) the sweep failed: window errors formed from
KOFF - 3 instead of KOFF - 4 in k_chunk's step 3 — 11 of the 15 360 (base, frame) placements differ (test_gpu_tail_prefix and
test_gpu_tail_selection pass on it); rank_excl's mask as (1 << (nb & 63)) - 1 — 3 549 placements differ (the two older files fail too)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import span_cases as sc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# seconds a child may take: five times its measured run time (0.87 s and 0.55 s at most, above), because the machine is shared
LIMIT_SWEEP, LIMIT_LOOP = 5, 3


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """The oracle's quads of every frame, once (they do not depend on the base), the conditions asserted; one .npz for all children."""
    fig, quads = sc.CONDITIONS["sweep"](oracle)
    cfig, cquads = sc.CONDITIONS["crowded"](oracle)
    data = {"f_crowded": sc.crowded_frames()}
    for i, q in enumerate(cquads):
        data["q_crowded_%d" % i] = q
    for sheet in sc.SHEETS:
        data["f_%d" % sheet] = sc.sweep_frames(sheet)
        for i, q in enumerate(quads[sheet]):
            data["q_%d_%d" % (sheet, i)] = q
    path = str(tmp_path_factory.mktemp("span_alignment") / "cases.npz")
    np.savez(path, **data)
    return path, dict(fig, **cfig)


_ended_badly = []   # children that were ended by a signal or their time limit
_runs = {}


def _child(path, names, bases, limit, **knobs):
    """(mismatches, hash, calls, completed process) of one child on the diagnostics build with the split fit forced"""
    assert not _ended_badly, "an earlier child did not end by itself: nothing more is started on the device: %s" % _ended_badly
    from conftest import diag_env
    env = diag_env(CK_FIT_FLAT="2", **knobs)
    env.pop("CK_EXT_BASE", None)
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(HERE, "span_alignment_child.py"), path, names, bases],
                       capture_output=True, text=True, env=env, timeout=limit + 60)
    wall = time.time() - t0
    if r.returncode not in (0, 1):
        _ended_badly.append((names, bases, r.returncode))
    out = {ln.split()[0]: ln.split()[1] for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ("CALLS", "MISMATCHES", "HASH", "SECONDS")}
    assert len(out) == 4, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(names, bases, knobs, out, "child's run time %.2f s of %d" % (wall, limit))
    return int(out["MISMATCHES"]), out["HASH"], int(out["CALLS"]), r


def _sweep(path, lo):
    if lo not in _runs:
        _runs[lo] = _child(path, ",".join(str(s) for s in sc.SHEETS), "%d:%d" % (lo, lo + 256), LIMIT_SWEEP)
    return _runs[lo]


@pytest.mark.parametrize("lo", [0, 256, 512, 768])
def test_one_cluster_at_every_base(cases, lo):
    """Every residue of e0, e1 and of every maximum modulo 960 (hence 64 and 32), the cluster starting in span 0 and in span 1."""
    assert set(range(0, 1024)) == set(sc.BASES)
    bad, _, calls, r = _sweep(cases[0], lo)
    assert calls == 2 * 256
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_one_cluster_at_the_span_starts_on_poisoned_buffers(cases):
    """A position read without having been written shows as a quad that differs (the handles' buffers start as 0xA5 bytes)."""
    assert sc.POISON_BASES == list(range(128)) + list(range(896, 1024))
    bad, _, calls, r = _child(cases[0], ",".join(str(s) for s in sc.SHEETS), "0:128,896:1024", LIMIT_SWEEP, CK_POISON="1")
    assert calls == 2 * 256
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("poison", [False, True])
def test_several_spans_per_workgroup(cases, poison):
    """k_chunk's loop (s += gridDim.x, the next span's points and weights fetched while this one is worked on) as the batch runs it:
    8 workgroups for the 128 and more spans of a crowded frame.  The order in which the clusters are placed stays free."""
    knobs = {"CK_POISON": "1"} if poison else {}
    bad, _, calls, r = _child(cases[0], "crowded", ",".join(str(b) for b in sc.LOOP_BASES), LIMIT_LOOP, CK_CHUNK_WGS="0", **knobs)
    assert calls == len(sc.LOOP_BASES) == 6
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_sweep_is_deterministic(cases):
    """The first sweep child's calls in a second process: the same hash over all quads."""
    first = _sweep(cases[0], 0)
    second = _child(cases[0], ",".join(str(s) for s in sc.SHEETS), "0:256", LIMIT_SWEEP)
    assert first[3] is not second[3] and first[1] == second[1] and second[0] == 0
