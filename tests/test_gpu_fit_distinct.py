"""GPU: the quad fit on distinct points (k_quads.hip: FitArgs::distinct — the sort leaves the (x, y) words, no tie-break, no search for
duplicates, the sequence's place asked for as soon as the border direction is accepted) against the path it replaces, in both
kernels.  Quads as sorted records, detections and status words, byte for byte against the oracle, on the frames whose twins sit
where the merge could fail (tests/test_fit_distinct_host.py shows that they do), at the edges of the size classes, on both paths of
the sort, with clusters that pass the size gate on fewer than 24 stored words, and in the two largest classes that sort in LDS:

  * the product library in this process: calls this small run the unsplit fit, k_fit;
  * child processes on the diagnostics build (tests/fit_distinct_child.py) with the split fit forced, k_seq: CK_FIT_FLAT=2; the same on
    poisoned buffers; with CK_EMIT_TWINS=2, which merges the twins but does not tell the fit, and with CK_EMIT_TWINS=0, which stores
    every point on its own — the two settings under which the retained path runs, with and without duplicates to find.

All of them must return the same bytes."""
import os
import subprocess
import sys

import pytest

import fit_distinct_cases as fd

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# class edge (points per cluster) -> threads per cluster of the class below it (tests/test_gpu_seq_front.py)
EDGES = {256: 64, 512: 64, 1024: 128, 2048: 256, 4096: 256}
SETTINGS = {"flat": dict(CK_FIT_FLAT="2"),
            "flat, fit not told": dict(CK_FIT_FLAT="2", CK_EMIT_TWINS="2"),
            "flat, no twins": dict(CK_FIT_FLAT="2", CK_EMIT_TWINS="0"),
            "flat, poisoned": dict(CK_FIT_FLAT="2", CK_POISON="1")}


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """the frames and the oracle's results for them, computed once and shared by every test: one .npz file"""
    path = str(tmp_path_factory.mktemp("fit_distinct") / "cases.npz")
    sizes, nquads = fd.save_cases(path, oracle)
    return path, sizes, nquads


def _assert_inputs(sizes, nquads):
    """Conditions on the inputs, checked on the oracle's clusters: without them the tests could pass without having run the code.
    (points, distinct coordinates) per kept cluster; the device files a cluster by its distinct coordinates when twins are merged
    (dedges704 straddles the class edges in that count) and by its points when they are not (edges640, edges272)."""
    for name, k in (("edges640", 0), ("edges272", 0), ("dedges704", 1)):
        counts = [s[k] for s in sizes[name]]
        for edge, nth in EDGES.items():
            if edge == 4096 and name == "edges272":
                continue   # 3 * (2 * 272 + 2 * 200) = 2 832 points at most in such a frame
            assert any(edge - nth < c <= edge for c in counts), f"{name}: no cluster just below {edge}: {sorted(counts)}"
            assert any(edge < c <= edge + nth for c in counts), f"{name}: no cluster just above {edge}: {sorted(counts)}"
        assert nquads[name] >= 4
    assert nquads["shapes640"] >= 3 and nquads["three640"] >= 5
    for gate in (24, 50):   # kept on its points, fewer stored words than the gate
        assert [(c, u < gate) for c, u in sizes[f"gate{gate}"]] == [(gate, True)], sizes[f"gate{gate}"]
    assert any(24 <= c <= 30 and u < 24 for c, u in sizes["gate24"])
    assert any(4096 < c <= 8192 for c, _ in sizes["large720"]) and any(8192 < c <= 16384 for c, _ in sizes["large720"]), sizes["large720"]
    assert any(8192 < u and c <= 16384 for c, u in sizes["large1280"]), sizes["large1280"]
    assert nquads["large720"] >= 1 and nquads["large1280"] >= 1
    assert sum(c - u for v in sizes.values() for c, u in v) > 20000   # duplicates for the retained path to find


def test_inputs_reach_the_class_edges_and_the_large_classes(cases):
    _assert_inputs(cases[1], cases[2])


@pytest.fixture(scope="module")
def product_run(cases):
    """in this process, on the product library"""
    import contextlib
    import io
    from fit_distinct_child import run
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        bad = run(cases[0])
    return bad, [ln.split()[1] for ln in out.getvalue().splitlines() if ln.startswith("HASH")][0], out.getvalue()


def test_k_fit_on_the_product_library(cases, product_run):
    _assert_inputs(cases[1], cases[2])
    assert product_run[0] == 0, product_run[2][-3000:]


_children = {}


def _child(path, setting):
    """the cases in a child process on the diagnostics build (its knobs are read once per process); the child's GPU work runs under a
    time limit of its own.  One run per setting, shared by the tests."""
    if setting not in _children:
        from conftest import diag_env
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(HERE, "fit_distinct_child.py"), path], capture_output=True,
                           text=True, env=diag_env(**SETTINGS[setting]), timeout=300)
        lines = r.stdout.splitlines()
        bad = [ln for ln in lines if ln.startswith("MISMATCHING_FRAMES")]
        hashes = [ln for ln in lines if ln.startswith("HASH")]
        assert bad and hashes, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        _children[setting] = (int(bad[0].split()[1]), hashes[0].split()[1], r)
    return _children[setting]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_k_seq_on_the_diagnostics_build(cases, setting):
    _assert_inputs(cases[1], cases[2])
    bad, _, r = _child(cases[0], setting)
    assert bad == 0 and r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_every_setting_returns_the_same_bytes(cases, product_run):
    hashes = {setting: _child(cases[0], setting)[1] for setting in SETTINGS}
    hashes["product"] = product_run[1]
    assert len(set(hashes.values())) == 1, hashes
