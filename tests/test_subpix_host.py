"""Sub-pixel corners on the host (ck_subpix_host.c, chalkydri_amd/subpix.py): the twins against the numpy
restatement (tests/np_subpix.py), their accuracy against the renderers' truth on AprilGrid frames (tests/np_board_render.py) and on
isolated tags (tests/np_tag_render.py) with the oracle's detections, board recovery, the contract's edges, the refusals, the struct
layouts and the host half under sanitizers.  No device needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_board_render as BR  # noqa: E402
import np_subpix as NS  # noqa: E402
import np_tag_render as NR  # noqa: E402
import subpix_scenes as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "chalkydri_amd", "lib", "subpix_host_check")


@pytest.fixture(scope="module")
def sp(built):
    from chalkydri_amd import subpix
    return subpix


@pytest.fixture(scope="module")
def A(built):
    from chalkydri_amd import _abi
    return _abi


def saddle(w=160, h=120, x=80, y=60, lo=0, hi=200):
    img = np.full((h, w), lo, np.uint8)
    img[:y, :x] = hi
    img[y:, x:] = hi
    return img


# ---- the twin against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 5, 7])
def test_twin_agrees_with_the_restatement(sp, oracle, w):
    """eps = 0: both sides take exactly max_iters steps, so no termination branch can flip.  Every point within 1e-6 px: three orders
    below eps, far above double rounding on sums of at most 225 terms.  Measured: 5e-14 px at most (w = 2, 5, 7; 32 points each)."""
    img, _ = SC.board_frame(2, 0.8)
    pts = np.concatenate([d["p"] for d in SC.board_dets(2, 0.8)] + [[[80.0, 60.0], [3.2, 4.1], [641.5, 479.2], [320.25, 240.75]]])
    pp = sp.subpix_params(half_win=w, eps=0.0)
    got, info = sp.corner_subpix_host(img, 0, pts, pp, return_info=True)
    want, st, it = NS.refine_many(img, pts, w=w, eps=0.0)
    assert np.array_equal(info["status"], st) and np.array_equal(info["iters"], it)
    moving = info["status"] != NS.FLAT
    assert moving.sum() >= len(pts) - 4 and (info["iters"][moving] == 30).all()
    diff = np.abs(got - want).max()
    print("w", w, "points", len(pts), "max |twin - numpy|", diff)
    assert diff <= 1e-6


def test_default_run_agrees_too(sp, oracle):
    """the default parameters (eps 1e-3): the same statuses and iteration counts, the points within 1e-6 px"""
    img, _ = SC.board_frame(1, 0.0)
    pts = np.concatenate([d["p"] for d in SC.board_dets(1, 0.0)])
    got, info = sp.corner_subpix_host(img, 0, pts, return_info=True)
    want, st, it = NS.refine_many(img, pts)
    assert np.array_equal(info["status"], st) and np.array_equal(info["iters"], it) and (st == NS.CONVERGED).all()
    assert np.abs(got - want).max() <= 1e-6
    assert np.allclose(info["shift"], np.linalg.norm(got - pts, axis=1), rtol=0, atol=1e-12)


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blur", SC.BLURS)
def test_aprilgrid_seed_corners_and_recovery(sp, oracle, blur):
    """(a) the refined seed corners' RMS error is at most half the detector's on the same corners; (b) recovery returns every tag of the
    board (all windows lie inside the frame; nothing is painted over); (c) the recovered corners' RMS error is at most half the
    detector's seed RMS.  Measured (detector / refined seeds / all recovered corners, px RMS; seeds of 64 tags):
    blur 0: 0.384 / 0.105 / 0.109, 34 seeds; blur 0.8: 0.358 / 0.079 / 0.087, 25 seeds; blur 1.5: 0.415 / 0.094 / 0.090, 13 seeds;
    64 of 64 tags recovered at every blur."""
    e_det, e_ref, e_all, n_seeds, n_known = [], [], [], 0, 0
    for seed in SC.SEEDS:
        img, truth = SC.board_frame(seed, blur)
        dets = SC.board_dets(seed, blur)
        seeds = SC.seeds_of(dets)
        assert seeds, "the view has no decoded tag to start from"
        p = np.array([d["p"] for d in seeds]).reshape(-1, 2)
        t = np.array([truth["uv"][d["id"]] for d in seeds]).reshape(-1, 2)
        e_det.append(p - t)
        e_ref.append(sp.corner_subpix_host(img, 0, p) - t)
        uv, state = sp.board_corners_host(SC.board(), img, [SC.records(dets)])
        assert set(np.nonzero(state[0] == 1)[0]) <= {d["id"] for d in seeds}
        assert (state[0] > 0).all(), f"view {seed}: tags {np.nonzero(state[0] == 0)[0].tolist()} not recovered"
        n_seeds += int((state[0] == 1).sum())
        n_known += int((state[0] > 0).sum())
        e_all.append((uv[0] - truth["uv"]).reshape(-1, 2))
    det, ref, rec = SC.rms(np.concatenate(e_det)), SC.rms(np.concatenate(e_ref)), SC.rms(np.concatenate(e_all))
    print(f"blur {blur}: detector {det:.3f} px RMS, refined seeds {ref:.3f}, recovered corners {rec:.3f}; {n_seeds} seeds, {n_known} of 64 tags")
    assert n_known == 64
    assert ref <= 0.5 * det
    assert rec <= 0.5 * det


def test_aprilgrid_with_a_painted_patch(sp, oracle):
    """A flat grey rectangle over the four middle tags: every tag clear of it is recovered, none under it.  Measured: 48 of 48, 0 false."""
    n_clear = n_false = 0
    for seed in SC.SEEDS:
        img, truth = SC.board_frame(seed, 0.8, True)
        assert truth["hidden"].sum() == 4 and truth["clear"].sum() == 12
        uv, state = sp.board_corners_host(SC.board(), img, [SC.records(SC.board_dets(seed, 0.8, True))])
        n_false += int((state[0][truth["hidden"]] > 0).sum())
        n_clear += int((state[0][truth["clear"]] > 0).sum())
        assert np.abs(uv[0][state[0] > 0] - truth["uv"][state[0] > 0]).max() < 0.6
        assert not uv[0][state[0] == 0].any()
    print("patched views:", n_clear, "of 48 clear tags recovered,", n_false, "hidden ones")
    assert n_false == 0 and n_clear == 48


def _isolated(oracle, sp, blur):
    from chalkydri_amd import _lib, default_config
    fam, cfg = _lib.family("tag36h11"), default_config(SC.W, SC.H)
    e_det, e_ref = [], []
    for seed in SC.SEEDS:
        img, truth = NR.scene([fam], seed, noise=0)
        f = img.astype(float)
        f = BR.gaussian_blur(f, blur) if blur > 0 else f
        f = f + np.random.default_rng(seed).normal(0, SC.noise_of(seed), f.shape)
        img = np.clip(np.rint(f), 0, 255).astype(np.uint8)
        by_id = {t["id"]: t["corners"] for t in truth}
        for d in oracle.detect(img, cfg)[0]:
            if d["hamming"] == 0 and d["id"] in by_id:
                e_det.append(d["p"] - by_id[d["id"]])
                e_ref.append(sp.corner_subpix_host(img, 0, d["p"]) - by_id[d["id"]])
    return len(e_det) * 4, SC.rms(np.concatenate(e_det)), SC.rms(np.concatenate(e_ref))


@pytest.mark.parametrize("blur", [0.0, 0.8])
def test_isolated_tags_are_not_made_worse(sp, oracle, blur):
    """Isolated tags (L-corners, not saddles): the refined RMS is not above the detector's.  Measured, 96 corners each: blur 0
    0.305 -> 0.216 px, blur 0.8 0.271 -> 0.217 px."""
    n, det, ref = _isolated(oracle, sp, blur)
    print(f"isolated tags, blur {blur}: {n} corners, detector {det:.3f} px RMS, refined {ref:.3f}")
    assert n >= 80 and ref <= det


def test_isolated_tags_under_heavy_blur_is_documented_behaviour(sp, oracle):
    """Blur sigma 1.5 with the default 11 x 11 window: the refinement is WORSE than the detector on L-corners (measured 0.225 ->
    0.388 px), which is why the setting is off by default and the window the caller's choice.  Not gated: the figures are printed."""
    n, det, ref = _isolated(oracle, sp, 1.5)
    print(f"isolated tags, blur 1.5: {n} corners, detector {det:.3f} px RMS, refined {ref:.3f}")
    assert n >= 80 and np.isfinite(ref)


# ---- contract ----------------------------------------------------------------------------------------------------------------------------
def test_flat_and_rejected_return_the_input_bytes(sp, A):
    flat = np.full((120, 160), 77, np.uint8)
    pts = np.array([[80.3, 60.9], [0.0, 0.0], [160.0, 120.0], [17.0, 5.5]])
    out, info = sp.corner_subpix_host(flat, 0, pts, return_info=True)
    assert out.tobytes() == pts.tobytes() and (info["status"] == A.CK_SUBPIX_FLAT).all() and not info["iters"].any() and not info["shift"].any()
    img = saddle()
    for w in (2, 5, 7):  # a corner just outside the window's reach pulls the point more than w away
        pts = np.array([[80 - w - 1.2, 59.0], [80 - w - 0.4, 58.0], [80 - w - 1.4, 60 - w - 1.4]])
        out, info = sp.corner_subpix_host(img, 0, pts, sp.subpix_params(half_win=w), return_info=True)
        assert (info["status"] == A.CK_SUBPIX_REJECTED).all() and out.tobytes() == pts.tobytes() and not info["shift"].any()
        assert (info["iters"] > 0).all()
        assert [NS.refine(img, x, y, w=w)[2] for x, y in pts] == [NS.REJECTED] * 3


def test_integer_points_and_points_near_every_edge(sp, A):
    img = saddle()
    out, info = sp.corner_subpix_host(img, 0, [[80.0, 60.0], [79.0, 61.0], [82.0, 58.0]], return_info=True)
    assert (info["status"] == A.CK_SUBPIX_CONVERGED).all() and np.abs(out - [80.0, 60.0]).max() < 1e-3
    # saddles 3 px from each edge and corner of the frame, windows of every size hanging over it: the clamp keeps the sampling defined
    for w in (2, 5, 7):
        pp = sp.subpix_params(half_win=w)
        for x, y in [(3, 60), (157, 60), (80, 3), (80, 117), (3, 3), (157, 3), (3, 117), (157, 117)]:
            im = saddle(x=x, y=y)
            pts = np.array([[x + 0.6, y - 0.7], [float(x), float(y)], [0.0, 0.0], [160.0, 120.0], [0.0, 120.0], [160.0, 0.0]])
            out, info = sp.corner_subpix_host(im, 0, pts, pp, return_info=True)
            want, st, it = NS.refine_many(im, pts, w=w)
            assert np.array_equal(info["status"], st) and np.abs(out - want).max() <= 1e-6
            assert info["status"][0] == A.CK_SUBPIX_CONVERGED and np.abs(out[0] - [x, y]).max() < 0.05


def test_weights(sp):
    for w in range(2, 8):
        m = sp.weights(sp.subpix_params(half_win=w))
        assert m.shape == (2 * w + 1, 2 * w + 1)
        assert np.array_equal(m, m.T) and np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1]) and m[w, w] == 1.0
        assert np.allclose(m, NS.weights(w), rtol=4e-16, atol=0)


def test_refusals(sp, A):
    from chalkydri_amd._lib import ChalkydriError
    img = saddle()

    def refused(fn, *a, **k):
        with pytest.raises(ChalkydriError) as e:
            fn(*a, **k)
        assert e.value.code == A.CK_EINVAL

    for bad in (dict(half_win=1), dict(half_win=8), dict(max_iters=0), dict(max_iters=1001), dict(eps=-1e-9), dict(eps=np.nan),
                dict(det_min=-1.0), dict(det_min=np.inf)):
        refused(sp.corner_subpix_host, img, 0, [[80.0, 60.0]], sp.subpix_params(**bad))
        refused(sp.weights, sp.subpix_params(**bad))
    for pt in ([np.nan, 5.0], [5.0, np.inf], [-0.01, 5.0], [160.01, 5.0], [5.0, -1e-9], [5.0, 120.5]):
        refused(sp.corner_subpix_host, img, 0, [[80.0, 60.0], pt])
    refused(sp.corner_subpix_host, img, 1, [[80.0, 60.0]])
    refused(sp.corner_subpix_host, img, [0, -1], [[80.0, 60.0], [80.0, 60.0]])
    assert sp.corner_subpix_host(img, 0, np.zeros((0, 2))).shape == (0, 2)  # n = 0 is a no-op
    from chalkydri_amd.calibration import Board
    for bad in (Board(9, 8), Board(65, 1)):
        refused(sp.board_corners_host, bad, img, [[]])
    refused(sp.board_corners_host, Board(4, 4), img, [[]], None, None, 4)
    refused(sp.board_corners_host, Board(4, 4), img, [[]], None, sp.board_params(agree=-1.0))
    uv, state = sp.board_corners_host(Board(4, 4), img, [[]])
    assert not state.any() and not uv.any()


def test_struct_layouts(A, sp):
    assert [(n, getattr(A.SubpixParams, n).offset) for n, _ in A.SubpixParams._fields_] == [("half_win", 0), ("max_iters", 4), ("eps", 8), ("det_min", 16)]
    assert [(n, getattr(A.SubpixInfo, n).offset) for n, _ in A.SubpixInfo._fields_] == [("status", 0), ("iters", 4), ("shift", 8)]
    assert [getattr(A.BoardDesc, n).offset for n, _ in A.BoardDesc._fields_] == [0, 4, 8, 12, 16, 24]
    assert [getattr(A.BoardParams, n).offset for n, _ in A.BoardParams._fields_] == [0, 8, 16, 32]
    assert (C.sizeof(A.SubpixParams), C.sizeof(A.SubpixInfo), C.sizeof(A.BoardDesc), C.sizeof(A.BoardParams)) == (24, 16, 32, 40)
    pp, bp = sp.subpix_params(), sp.board_params()
    assert (pp.half_win, pp.max_iters, pp.eps, pp.det_min) == (5, 30, 1e-3, 1e-2)
    assert (bp.seed_max_shift, bp.max_shift, bp.probe[0], bp.probe[1], bp.agree) == (2.0, 2.5, 0.7, -0.6, 0.05)
    assert (A.CK_SUBPIX_CONVERGED, A.CK_SUBPIX_MAXIT, A.CK_SUBPIX_FLAT, A.CK_SUBPIX_REJECTED) == (0, 1, 2, 3)


def test_host_half_under_sanitizers(built):
    """csrc/ck_subpix_host.c alone under AddressSanitizer + UBSan, driven by tests/cpp/subpix_host_check.cpp: points on the frame
    border and in its corners, n = 0, w = 2 and w = 7, a board at the frame edge."""
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "subpix_host_check ok" in r.stdout
