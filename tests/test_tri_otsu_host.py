"""The iterative tri-class Otsu threshold without a GPU: ck_tri_otsu_solve byte for byte against the restatement in
Python integers and floats (tests/np_tri_otsu.py), the restatement against the independent exact solver in fractions, every
refusal, and the gray map.

Near-ties.  Restatement and exact solver may differ only where fp64 rounding reorders two v(t) whose exact relative gap is below
2^-40; such a case is left out of that comparison, at most 1 % of the random ones and none of the fixed ones.  The rule here is
stricter than that: an exact tie (gap 0) is NOT left out, the smallest-t rule must decide it in both.  Observed with seed 20141:
0 of 400 random cases left out, 0 of the fixed ones.

The stop `lo' > hi'`.  The contract keeps it, and both solvers implement it, but no histogram reaches it: the lower class mean is
at most T_k and the upper one at least T_k + 1, so lo' = ceil(mu0) <= T_k < T_k + 1 <= floor(mu1) = hi'.  A two-level region {a, b}
gives T = a, lo' = a, hi' = b: the interval collapses ONTO the two levels and the next round stops on the repeated T.  For the same
reason a later round never finds fewer than two occupied levels: the highest occupied level of the lower class is >= ceil(mu0) and
the lowest of the upper class <= floor(mu1), so both stay inside.  Every run therefore ends on a repeated T or on max_iters.  The
fixed cases hold those regions (adjacent levels too) and the tests assert what can be observed: lo_final <= T_last < hi_final, and
the last round is a repeat or round max_iters, in every case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_tri_otsu as N  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

SEED, N_RANDOM = 20141, 400
TOTAL_MAX = 1 << 27        # S n and N s stay below 2^63 while the pixel count stays below 2^27.5


def _scaled(w):
    """float weights -> counts whose largest is at most 2^24 and whose sum is at most TOTAL_MAX"""
    w = np.maximum(np.asarray(w, np.float64), 0)
    top = min(float(1 << 24), TOTAL_MAX * w.max() / max(w.sum(), 1e-300))
    return np.floor(w * (top / max(w.max(), 1e-300))).astype(np.uint32)


def random_hist(rng, case):
    g = np.arange(256)
    kind = case % 5
    if kind == 0:                                                   # sparse: a few levels, counts up to 2^24
        h = np.zeros(256, np.uint32)
        lv = rng.choice(256, int(rng.integers(2, 9)), replace=False)
        h[lv] = rng.integers(1, (1 << 24) + 1, lv.size)
        return h
    bump = lambda: np.exp(-0.5 * ((g - rng.uniform(0, 255)) / rng.uniform(1.5, 30)) ** 2) * rng.uniform(0.2, 1)
    if kind == 1:
        return _scaled(bump() + bump())
    if kind == 2:
        return _scaled(bump() + bump() + bump() + rng.uniform(0, 1e-3))
    if kind == 3:                                                   # heavy-tailed counts on every level
        return _scaled(rng.pareto(0.7, 256))
    h = rng.integers(0, 1 << int(rng.integers(1, 20)), 256).astype(np.uint32)   # small counts, many exact coincidences
    h[rng.random(256) < rng.uniform(0, 0.9)] = 0
    return h


def _two(a, x, b, y):
    h = np.zeros(256, np.uint32)
    h[a], h[b] = x, y
    return h


def fixed_hists():
    out = {"empty": np.zeros(256, np.uint32), "one level": _two(77, 1000, 77, 1000), "one level at 0": _two(0, 5, 0, 5),
           "two levels": _two(10, 300, 200, 500), "two adjacent levels": _two(99, 7, 100, 9), "two levels at the ends": _two(0, 1, 255, 1),
           "two adjacent at the top": _two(254, 1 << 24, 255, 3), "all levels equal": np.full(256, 1000, np.uint32),
           "all levels equal, large": np.full(256, 1 << 19, np.uint32)}
    h = np.zeros(256, np.uint32)                                    # a region that collapses onto two adjacent levels: the narrowest there is
    h[[94, 100, 101, 108]] = [1, 1000, 1000, 1]
    out["collapse onto two adjacent levels"] = h
    h = np.zeros(256, np.uint32)
    h[[0, 127, 128, 129, 255]] = [50, 1, 1, 1, 50]
    out["three thin levels between two heavy ones"] = h
    h = np.zeros(256, np.uint32)
    h[40:60], h[180:230], h[100:140] = 900, 700, 30
    out["tag-like: two plateaus and a thin middle"] = h
    return out


PARAMS = ({}, {"keep_tbd": 0}, {"max_iters": 1}, {"max_iters": 1, "keep_tbd": 0}, {"min_delta": 255}, {"min_delta": 255, "keep_tbd": 0},
          {"max_iters": 32, "min_delta": 1}, {"max_iters": 3, "min_delta": 4})


@pytest.fixture(scope="module")
def cases():
    """(name, hist, params, restatement's (record, table)) of every fixed and random case: computed once, shared, left unchanged"""
    rng = np.random.default_rng(SEED)
    out = []
    for name, h in fixed_hists().items():
        for kw in PARAMS:
            out.append((name, h, kw, N.solve(h, **kw)))
    for i in range(N_RANDOM):
        h = random_hist(rng, i)
        assert int(h.sum(dtype=np.uint64)) <= TOTAL_MAX and int(h.max()) <= 1 << 24
        kw = PARAMS[int(rng.integers(0, len(PARAMS)))] if i % 2 else {"max_iters": int(rng.integers(1, 33)), "min_delta": int(rng.integers(1, 6)),
                                                                      "keep_tbd": int(rng.integers(0, 2))}
        out.append(("random %d" % i, h, kw, N.solve(h, **kw)))
    return out


def test_library_equals_the_restatement(built, cases):
    from chalkydri_amd.cat import TRI_INFO_DTYPE, tri_otsu_solve
    assert TRI_INFO_DTYPE == N.INFO_DTYPE
    for name, h, kw, (want_info, want_lut) in cases:
        info, lut = tri_otsu_solve(h, **kw)
        assert info.tobytes() == want_info.tobytes(), (name, kw, info, want_info)
        assert lut.tobytes() == want_lut.tobytes(), (name, kw)
        assert int(info["n_black"]) + int(info["n_white"]) + int(info["n_other"]) == int(h.sum(dtype=np.uint64))
        if kw.get("keep_tbd", 1) == 0:
            assert int(info["n_other"]) == 0 and OTHER_FREE(lut)


def OTHER_FREE(lut):
    return not np.any(lut == N.OTHER)


def test_restatement_equals_the_exact_solver(cases):
    left_out = {"fixed": 0, "random": 0}
    for name, h, kw, (info, lut) in cases:
        ex = N.solve_exact(h, **kw)
        kind = "random" if name.startswith("random") else "fixed"
        if ex["min_gap"] is not None and 0 < ex["min_gap"] < 2.0 ** -40:
            left_out[kind] += 1
            continue
        r = int(info["n_rounds"])
        assert [int(t) for t in info["T"][:r]] == ex["T"] and np.all(info["T"][r:] == -1), (name, kw)
        assert lut.tobytes() == ex["lut"].tobytes(), (name, kw)
        if r:
            assert (int(info["lo_final"]), int(info["hi_final"])) == (ex["lo"], ex["hi"]), (name, kw)
            assert int(info["lo_final"]) <= int(info["T_last"]) < int(info["hi_final"])     # (the docstring's lo' <= T < hi')
            assert r == kw.get("max_iters", 8) or abs(int(info["T"][r - 1]) - int(info["T"][r - 2])) < kw.get("min_delta", 1)
        else:
            assert int(info["flags"]) == N.FLAT and (int(info["T_last"]), int(info["lo_final"]), int(info["hi_final"])) == (-1, 0, 255)
    print("left out as near-ties:", left_out)
    assert left_out["fixed"] == 0 and left_out["random"] <= N_RANDOM // 100


def test_fixed_cases_mean_what_their_names_say(cases):
    by = {(name, tuple(sorted(kw.items()))): out for name, _, kw, out in cases}
    d = lambda name, **kw: by[(name, tuple(sorted(kw.items())))]
    for name in ("empty", "one level", "one level at 0"):
        for kw in ({}, {"keep_tbd": 0}):
            info, lut = d(name, **kw)
            assert int(info["n_rounds"]) == 0 and int(info["flags"]) == N.FLAT and np.array_equal(lut, (np.arange(256) >= 128).astype(np.uint8))
    info, lut = d("two levels")
    assert int(info["n_rounds"]) == 2 and list(info["T"][:2]) == [10, 10] and (int(info["lo_final"]), int(info["hi_final"])) == (10, 200)
    info, lut = d("two adjacent levels")
    assert list(info["T"][:2]) == [99, 99] and lut[99] == N.OTHER and lut[100] == N.OTHER and lut[98] == N.BLACK and lut[101] == N.WHITE
    info, lut = d("two adjacent levels", keep_tbd=0)
    assert lut[99] == N.BLACK and lut[100] == N.WHITE
    info, _ = d("all levels equal")                                  # v(t) = v(254 - t): the smallest t of the tie wins
    assert int(info["T"][0]) == 127
    info, _ = d("all levels equal", max_iters=1)
    assert int(info["n_rounds"]) == 1 and (int(info["lo_final"]), int(info["hi_final"])) == (64, 191)
    info, lut = d("collapse onto two adjacent levels")
    assert (int(info["lo_final"]), int(info["hi_final"]), int(info["n_rounds"])) == (100, 101, 2) and lut[94] == N.BLACK and lut[108] == N.WHITE
    info, _ = d("two levels", min_delta=255)                         # any second threshold is a repeat
    assert int(info["n_rounds"]) == 2


def test_refusals(built):
    from chalkydri_amd.cat import tri_otsu_params
    from chalkydri_amd.detector import _bind
    from chalkydri_amd._lib import lib
    L = _bind(lib())
    h, info, lut = np.full(256, 3, np.uint32), A.TriOtsuInfo(), np.zeros(256, np.uint8)
    call = lambda p, hist=h.ctypes.data, i=C.byref(info), t=lut.ctypes.data: L.ck_tri_otsu_solve(p, hist, i, t)
    ok = tri_otsu_params()
    assert (ok.max_iters, ok.min_delta, ok.keep_tbd, ok.channels) == (8, 1, 1, 3)
    assert call(C.byref(ok)) == A.CK_OK
    assert call(None) == A.CK_EINVAL and call(C.byref(ok), hist=None) == A.CK_EINVAL
    assert call(C.byref(ok), i=None) == A.CK_EINVAL and call(C.byref(ok), t=None) == A.CK_EINVAL
    for field, bad in (("max_iters", (0, 33, -1)), ("min_delta", (0, 256)), ("keep_tbd", (2, -1)), ("channels", (0, 2, 4))):
        for v in bad:
            p = tri_otsu_params(**{field: v})
            assert call(C.byref(p)) == A.CK_EINVAL, (field, v)
    for kw in ({"max_iters": 1}, {"max_iters": 32}, {"min_delta": 255}, {"keep_tbd": 0}, {"channels": 1}):
        assert call(C.byref(tri_otsu_params(**kw))) == A.CK_OK, kw
    L.ck_tri_otsu_params_default(None)                               # a null pointer is ignored


def test_gray_map_of_cat_py_is_the_restatements():
    from chalkydri_amd.cat import grayscale
    v = np.arange(256, dtype=np.uint8)
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    a, bb = grayscale(r, g, b), N.gray(r, g, b)
    assert a.dtype == np.uint8 and a.shape == (256, 256, 256) and np.array_equal(a, bb)
    for c in ((0, 0, 0), (255, 255, 255), (200, 100, 50), (1, 2, 3)):   # the scalar form is unchanged
        assert isinstance(grayscale(*c), int) and grayscale(*c) == int(a[c])
    assert int(a[255, 255, 255]) == 252 and int(a.max()) == 252          # 0.33 * 3 < 1: the map never reaches 253
