"""CPU: the twin encoding of the packed boundary point (chalkydri_amd/csrc/ck_point.h).  ck_unpack_point + ck_unpack_twin of all
eight merged words reproduce the two points the oracle's emit rule makes of the 2 x 2 block, and ck_stage_point carries the sum of
their gradients (tests/cpp/twin_points_check.cpp, a host-only program)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_twin_encodings_reproduce_both_points(tmp_path):
    exe = str(tmp_path / "twin_points_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "chalkydri_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "twin_points_check.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


def test_twin_frames_reach_what_they_are_named_for(oracle):
    """The hand-drawn frames of tests/test_gpu_twin_points.py, by the oracle alone: the tile frames have twins on the emit-tile
    boundary itself, the rim frames single points where the other copy has no emitting owner, the checkerboards twins without one
    kept cluster (2 x 2 cells) or in hundreds of them (3 x 3), the staircase none; the gate shapes have exactly the counts they are
    filed under, and fewer distinct coordinates."""
    import cluster_cases as cc
    import twin_cases as tc
    frames = tc.edge_frames()
    for mcp in tc.EDGE_MIN_COMPONENT:
        want = {name: cc.oracle_clusters(oracle, f, mcp) for name, f in frames.items()}
        dup = {name: set().union(*tc.duplicates(w).values()) if w else set() for name, w in want.items()}
        pts = {name: {(int(r[0]), int(r[1])) for a in w.values() for r in a} for name, w in want.items()}
        assert {p[0] for p in dup["tile v63|64"]} == {127} and len(dup["tile v63|64"]) >= 90
        assert {p[1] for p in dup["tile h15|16"]} == {31} and len(dup["tile h15|16"]) >= 150
        assert len(want["tile cross"]) == 2 and (127, 33) in dup["tile cross"] and (129, 31) in dup["tile cross"]
        for name in ("rim h1|2", "rim h93|94", "rim h94|95"):   # the first and the last point of the row have no twin: its owner is column 0 / w - 1
            xs = sorted(p[0] for p in pts[name])
            assert xs[0] == 1 and not any(p[0] == 1 for p in dup[name]) and any(p[0] == 3 for p in dup[name]), name
            assert not any(p[0] == xs[-1] for p in dup[name]) and xs[-1] >= 2 * tc.W - 4, name
        assert {p[0] for p in dup["rim v1|2"]} == {3} and {p[0] for p in dup["rim v157|158"]} == {2 * tc.W - 5}
        assert not want["mixed checker2"] and not dup["mixed staircase"] and len(pts["mixed staircase"]) > 300
    for name in ("rim v0|1", "rim v158|159", "mixed checker2"):   # at min_component_px = 1 these have points, in clusters too small to keep
        logical, physical = tc.totals(oracle, frames[name], 1)
        assert logical > 90 and (physical < logical) == (name == "mixed checker2"), name
    assert len(cc.oracle_clusters(oracle, frames["mixed checker3"], 1)) > 500
    for gate, (dropped, kept) in tc.GATES.items():
        sizes = tc.cluster_sizes(oracle, tc.gate_frame(gate))
        assert [s[0] for s in sizes] == [dropped, kept] and all(s[1] < gate and s[1] < s[0] for s in sizes), (gate, sizes)
