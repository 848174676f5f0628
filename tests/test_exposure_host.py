"""The exposure meter without a GPU: the two numpy restatements against each other, the library's tables, metric
and recommendation against them, every refusal, and the closed loop on the CPU: a controller fed the restatement's statistics
settles near the best exposure from 8x under and 8x over, and the oracle detector finds there the tags it loses at the start."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exposure_scenes as S  # noqa: E402
import np_exposure as N  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402


def test_the_two_restatements_agree():
    lut = N.luts()
    rng = np.random.default_rng(5)
    for w, h, roi in ((37, 23, None), (16, 16, (3, 2, 11, 16)), (50, 19, (-4, -4, 60, 60)), (24, 31, (5, 5, 5, 9)), (20, 20, (0, 0, 1, 20)),
                      (33, 18, (30, 1, 40, 17))):
        for amp in (2, 16, 255):
            f = np.clip(100 + rng.integers(-amp, amp + 1, (h, w)), 0, 255).astype(np.uint8)
            a, b = N.stats(f, lut, roi), N.stats_loops(f, lut, roi)
            assert a.tobytes() == b.tobytes(), (w, h, roi, amp)
            assert int(a["luma"].sum()) == int(a["n_luma"]) and all(int(a["grad"][k].sum()) == int(a["n_grad"]) for k in range(N.GAMMAS))
    # the largest magnitude: a corner of 255 against 0 reaches S = 2 080 800, bin 180
    f = np.zeros((3, 3), np.uint8)
    f[0, 1:] = f[1, 2] = 255
    assert int(np.nonzero(N.stats_loops(f, lut)["grad"][3])[0][0]) == math.isqrt(2 * 765 * 765) >> 3
    f[:] = 0
    f[:, 2] = 255
    assert int(np.nonzero(N.stats(f, lut)["grad"][3])[0][0]) == 1020 >> 3


def test_luts(built):
    from chalkydri_amd.exposure import ExposureParams
    for gammas in (N.DEFAULT_GAMMAS, (0.2, 0.4, 0.7, 0.9, 1.0, 2.5, 4.0), (0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0)):
        got, want, real = ExposureParams(gamma=gammas).luts(), N.luts(gammas), N.lut_real(gammas)
        clear = np.abs(real + 0.5 - np.rint(real + 0.5)) > 1e-9          # not within 1e-9 of a tie
        clear[:, 0] = clear[:, 255] = True
        assert np.array_equal(got[clear], want[clear]) and clear.mean() > 0.99
        assert np.all(got[:, 0] == 0) and np.all(got[:, 255] == 255)
        assert np.all(np.diff(got.astype(int), axis=1) >= 0)
        assert np.array_equal(got[gammas.index(1.0)], np.arange(256))


def _adversarial():
    out = {}
    for name, fill in (("one bin", lambda g: g.__setitem__((slice(None), 57), 1000)),
                       ("empty", lambda g: None),
                       ("maximum at the low end", lambda g: [g.__setitem__((k, 100), 1000 - 100 * k) or g.__setitem__((k, 0), 100 * k) for k in range(7)]),
                       ("maximum at the high end", lambda g: [g.__setitem__((k, 100), 100 * k + 100) or g.__setitem__((k, 0), 900 - 100 * k) for k in range(7)]),
                       ("flat triple", lambda g: [g.__setitem__((k, 90), (500, 600, 700, 700, 700, 600, 500)[k]) or
                                                  g.__setitem__((k, 0), 1000 - (500, 600, 700, 700, 700, 600, 500)[k]) for k in range(7)]),
                       ("interior peak", lambda g: [g.__setitem__((k, 120), (300, 500, 640, 700, 690, 560, 400)[k]) or
                                                    g.__setitem__((k, 3), 1000 - (300, 500, 640, 700, 690, 560, 400)[k]) for k in range(7)])):
        s = np.zeros((), N.STATS_DTYPE)
        fill(s["grad"])
        s["n_grad"] = int(s["grad"][0].sum())
        out[name] = s
    return out


def test_metric_and_recommendation(built):
    from chalkydri_amd.exposure import ExposureParams, metric, recommend
    cases = _adversarial()
    rad, _ = S.radiance(1)
    lut = N.luts()
    for e in (0.3, 1.0, 3.0, 12.0):
        cases[f"scene at {e}"] = N.stats(N.photograph(rad, e), lut)
    cases["scene, a rectangle"] = N.stats(N.photograph(rad, 1.0), lut, (100, 50, 400, 300))
    rel = lambda a, b: abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    for kw in ({}, {"lam": 10.0, "delta": 0.0, "kp": 0.5, "e_min": 0.5, "e_max": 2.0}, {"gamma": (0.2, 0.4, 0.7, 0.9, 1.0, 2.5, 4.0), "delta": 0.3}):
        p, q = ExposureParams(**kw), N.Params(**kw)
        for name, s in cases.items():
            assert all(rel(a, b) for a, b in zip(metric(s, p), N.metric(q, s))), name
            for e0 in (0.01, 1.0, 250.0):
                (e, g), (e_ref, g_ref) = recommend(s, e0, p), N.recommend(q, s, e0)
                assert rel(e, e_ref) and rel(g, g_ref), (name, e0)
    p = N.Params()
    assert N.recommend(p, cases["empty"], 3.0) == (3.0, 1.0) and N.recommend(p, cases["one bin"], 3.0) == (3.0, 1.0)
    assert N.recommend(p, cases["maximum at the low end"], 1.0)[1] == p.gamma[0]
    assert N.recommend(p, cases["maximum at the high end"], 1.0)[1] == p.gamma[6]
    assert p.gamma[1] <= N.recommend(p, cases["flat triple"], 1.0)[1] <= p.gamma[3]
    assert recommend(cases["maximum at the low end"], 2.0)[0] > 2.0      # a best gamma below 1: brighten


def test_refusals(built):
    from chalkydri_amd.detector import _bind
    from chalkydri_amd.exposure import ExposureParams
    from chalkydri_amd._lib import lib
    L = _bind(lib())
    s, m, lut = A.ExposureStats(), (C.c_double * 7)(), (C.c_uint8 * (7 * 256))()
    nxt, g = C.c_double(), C.c_double()

    def rcs(p, e=1.0):
        return (L.ck_exposure_luts(C.byref(p.c), lut), L.ck_exposure_metric(C.byref(p.c), C.byref(s), m),
                L.ck_exposure_recommend(C.byref(p.c), C.byref(s), e, C.byref(nxt), C.byref(g)))
    assert rcs(ExposureParams()) == (0, 0, 0)
    bad = [("lambda_", 0.0), ("lambda_", -1.0), ("lambda_", math.inf), ("delta", -0.01), ("delta", 1.0), ("delta", math.nan), ("kp", 0.0),
           ("kp", math.nan), ("e_min", 0.0), ("e_max", math.inf), ("e_min", 2e6)]
    for field, v in bad:
        p = ExposureParams()
        setattr(p.c, field, v)
        assert rcs(p) == (A.CK_EINVAL,) * 3, (field, v)
    for k, v in ((0, 0.0), (0, -1.0), (3, math.nan), (6, math.inf), (2, 1.0), (4, 0.9)):    # not positive, not finite, not increasing
        p = ExposureParams()
        p.c.gamma[k] = v
        assert rcs(p) == (A.CK_EINVAL,) * 3, (k, v)
    p = ExposureParams()
    for e in (0.0, -1.0, math.nan, math.inf):
        assert rcs(p, e)[2] == A.CK_EINVAL
    assert L.ck_exposure_luts(None, lut) == A.CK_EINVAL and L.ck_exposure_luts(C.byref(p.c), None) == A.CK_EINVAL
    assert L.ck_exposure_metric(C.byref(p.c), None, m) == A.CK_EINVAL and L.ck_exposure_metric(C.byref(p.c), C.byref(s), None) == A.CK_EINVAL
    assert L.ck_exposure_recommend(C.byref(p.c), C.byref(s), 1.0, None, None) == A.CK_EINVAL
    assert L.ck_exposure_recommend(C.byref(p.c), C.byref(s), 1.0, C.byref(nxt), None) == 0
    with pytest.raises(Exception):
        from chalkydri_amd.exposure import ExposureController
        ExposureController(ExposureParams(kp=-1.0), 1.0)


def test_roi_from_detections():
    from chalkydri_amd.exposure import roi_from_detections

    class D:
        def __init__(self, p):
            self.p = np.array(p, float)

        def corners(self):
            return self.p
    assert roi_from_detections([], 10, 640, 480) == (0, 0, 640, 480)
    d = [D([(100.5, 50.2), (140.9, 52.0), (139.0, 90.7), (99.1, 88.0)]), D([(300, 200), (320, 200), (320, 220), (300, 220)])]
    assert roi_from_detections(d, 0, 640, 480) == (99, 50, 321, 221)
    assert roi_from_detections(d, 16, 640, 480) == (83, 34, 337, 237)
    assert roi_from_detections(d, 500, 640, 480) == (0, 0, 640, 480)


def test_closed_loop_settles_and_finds_the_tags(built, oracle):
    """Measured with the numpy restatement: from E* / 8 and from 8 E* the controller is inside |ln(E / E*)| <= 0.9124
    after 10 steps and stays there (exposure_scenes.STEPS, BAND); asserted at twice the steps and 1.5 times the band.  The band is
    wide because the controller's fixed point, where the gamma sweep peaks at gamma 1, lies at 0.40-0.48 E* on this scene: the
    brute-force optimum E* gains gradient from clipping the grey panel, which a gamma curve with fixed end points cannot imitate."""
    from chalkydri_amd import default_config
    from chalkydri_amd.exposure import ExposureController
    rad, truth = S.radiance(1)
    e_star = S.best_exposure(rad)
    lut = N.luts()
    cfg = default_config(S.W, S.H)
    ids = sorted(t["id"] for t in truth)
    found = lambda e: sorted(d["id"] for d in oracle.detect(N.photograph(rad, e), cfg)[0] if d["id"] in ids)
    for start in (e_star / 8, e_star * 8):
        c = ExposureController(None, start)
        for _ in range(2 * S.STEPS):
            c.update(N.stats(N.photograph(rad, c.exposure), lut))
        for _ in range(10):
            assert abs(math.log(c.exposure / e_star)) <= 1.5 * S.BAND
            c.update(N.stats(N.photograph(rad, c.exposure), lut))
        assert found(c.exposure) == ids
    assert len(found(e_star / 8)) < len(ids)
