"""Iterative tri-class Otsu on the device: ck_cat_tri_otsu_batch byte-equal to the restatement
(tests/np_tri_otsu.py) over the smallest shapes at which each kernel can go wrong (one pixel, one 16-pixel piece, a piece plus
a ragged pixel, pieces that straddle rows, more than one workgroup), both channel counts, batches, and contents that stress the
histogram (flat: every lane on one bin), the solve (two levels, all levels equal: the tie rule) and the look-up; frames of a batch
independent of their neighbours; device pointers equal to host pointers; sentinels untouched; the CAT stages on the class map;
refusals; a helping of the stress script; and the same file once more on the diagnostics library with poisoned allocations."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_tri_otsu as N  # noqa: E402
import stress_tri_otsu as S  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402
from chalkydri_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (5, 3), (16, 1), (17, 2), (37, 21), (64, 48), (130, 67))
CONTENTS = ("random", "flat", "two levels", "all levels", "tags")


@pytest.fixture(scope="module")
def det(built):
    from chalkydri_amd.cat import CatDetector
    d = CatDetector(64, 48)
    yield d
    d.close()


@pytest.fixture(scope="module")
def scene():
    """one rendered tag scene, cropped by the cases that want it (left unchanged)"""
    g = synth.render(synth.frame_seed(5, 3), 320, 240, 3, min_side=40, max_side=110, noise_amp=2)[0]
    g.setflags(write=False)
    return g


def _frame(kind, w, h, ch, seed, scene):
    """[h][w][ch]"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w, ch), 201, np.uint8)
    if kind == "two levels":
        g = np.where(rng.random((h, w)) < 0.4, 30, 220).astype(np.uint8)
        g.flat[0], g.flat[-1] = 30, 220                  # (both present whenever there are two pixels)
    elif kind == "all levels":                           # all 256 values equally often where the size allows: every gray level the map reaches
        g = (np.arange(w * h) % 256).astype(np.uint8).reshape(h, w)
    else:
        y0, x0 = 60 + seed % 7, 40 + seed % 11
        g = np.ascontiguousarray(scene[y0:y0 + h, x0:x0 + w])
    return np.repeat(g[..., None], ch, axis=2)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("ch", (1, 3))
def test_batch_equals_the_restatement(det, scene, w, h, ch):
    for n in (1, 3):
        for kind in CONTENTS:
            frames = np.stack([_frame(kind, w, h, ch, 7 * w + h + i, scene) for i in range(n)])
            for kw in ({}, {"keep_tbd": 0, "max_iters": 3}):
                got = det.tri_otsu_batch(frames, **kw)
                assert S.mismatches(frames, got, kw) == 0, (kind, n, kw)
                if kw.get("keep_tbd", 1) == 0:
                    assert not np.any(got[0] == N.OTHER)


def test_all_levels_frame_is_what_it_says(scene):
    """the content generator's claim: the 256 values land on the 253 levels 0..252 (0.33 * 3 < 1), 4 or 8 pixels each"""
    for ch in (1, 3):
        h = N.histogram(N.gray_frame(_frame("all levels", 256, 4, ch, 0, scene)))
        assert np.count_nonzero(h) == 253 and h[253:].sum() == 0 and set(np.unique(h[:253])) == {4, 8}


def test_frames_do_not_depend_on_their_neighbours(det, scene):
    w, h = 130, 67
    frames = np.stack([_frame(k, w, h, 3, 5 + i, scene) for i, k in enumerate(("tags", "flat", "random"))])
    together = det.tri_otsu_batch(frames)
    for i in range(3):
        alone = det.tri_otsu_batch(frames[i:i + 1])
        assert all(a[i].tobytes() == b[0].tobytes() for a, b in zip(together, alone)), i
    swapped = det.tri_otsu_batch(frames[::-1])
    assert all(a[::-1].tobytes() == b.tobytes() for a, b in zip(together, swapped))


def test_device_pointers_equal_host_pointers(det, scene):
    import torch
    for (w, h), ch in (((130, 67), 3), ((17, 2), 1), ((64, 48), 3)):
        frames = np.stack([_frame(k, w, h, ch, 11 + i, scene) for i, k in enumerate(("tags", "random", "two levels"))])
        host = det.tri_otsu_batch(frames)
        dev = S.to_numpy(det.tri_otsu_batch(torch.from_numpy(frames).cuda()))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(host, dev)), (w, h, ch)
        # an unaligned device view: the frames start one byte into an allocation
        raw = torch.zeros(frames.size + 1, dtype=torch.uint8, device="cuda")
        raw[1:] = torch.from_numpy(frames.reshape(-1)).cuda()
        dev = S.to_numpy(det.tri_otsu_batch(raw[1:].view(frames.shape)))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(host, dev)), (w, h, ch)


def test_sentinels_stay_untouched(det, scene):
    import torch
    from chalkydri_amd.cat import tri_otsu_params
    for (w, h), n in (((17, 2), 3), ((130, 67), 2), ((1, 1), 1)):
        frames = np.stack([_frame("random", w, h, 3, 3 + i, scene) for i in range(n)])
        want = det.tri_otsu_batch(frames)
        p = tri_otsu_params()
        # host arrays with 64 sentinel bytes behind classes_out and hist_out
        cls, hist = np.full(n * w * h + 64, 0xEE, np.uint8), np.full(n * 256 + 16, 0xEEEEEEEE, np.uint32)
        assert det._L.ck_cat_tri_otsu_batch(det._det._h, C.byref(p), frames.ctypes.data, n, w, h, cls.ctypes.data, None, hist.ctypes.data) == 0
        assert cls[:n * w * h].tobytes() == want[0].tobytes() and np.all(cls[n * w * h:] == 0xEE)
        assert hist[:n * 256].tobytes() == want[2].tobytes() and np.all(hist[n * 256:] == 0xEEEEEEEE)
        # the same on the device, where the classes are written in place by the kernel
        dcls = torch.full((n * w * h + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        dhist = torch.full((n * 256 + 16,), -286331154, dtype=torch.int32, device="cuda")   # 0xEEEEEEEE
        dpx = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        assert det._L.ck_cat_tri_otsu_batch(det._det._h, C.byref(p), dpx.data_ptr(), n, w, h, dcls.data_ptr(), None, dhist.data_ptr()) == 0
        c, hh = dcls.cpu().numpy(), dhist.cpu().numpy().view(np.uint32)
        assert c[:n * w * h].tobytes() == want[0].tobytes() and np.all(c[n * w * h:] == 0xEE)
        assert hh[:n * 256].tobytes() == want[2].tobytes() and np.all(hh[n * 256:] == 0xEEEEEEEE)


def test_cat_stages_follow_the_class_map(det, scene):
    """CatDetector.tri_otsu keeps the classes as the detector's class map: detect_corners / connected_components return what the
    C entry points return for that map handed to them directly."""
    w, h = 64, 48
    g = synth.render(synth.frame_seed(5, 1), w, h, 1, min_side=24, max_side=40, noise_amp=2)[0]
    rgb = np.repeat(g[..., None], 3, axis=2)
    cls = det.tri_otsu(rgb).copy()
    want, info, _ = N.classify(rgb)
    assert np.array_equal(cls, want) and det.tri_info.tobytes() == info.tobytes()
    assert len(np.unique(cls)) >= 2
    pts = det.detect_corners()
    uf = det.connected_components()
    L, hd = det._L, det._det._h
    p2, n2 = np.zeros((w * h, 2), np.uint32), C.c_int32(0)
    assert L.ck_cat_detect_corners(hd, want.ctypes.data, w, h, p2.ctypes.data, w * h, C.byref(n2)) == 0
    assert np.array_equal(pts, p2[:n2.value])
    roots, sizes = np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32)
    assert L.ck_cat_connected_components(hd, want.ctypes.data, w, h, roots.ctypes.data, sizes.ctypes.data) == 0
    assert np.array_equal(uf._roots, roots.reshape(-1)) and np.array_equal(uf._sizes, sizes.reshape(-1))
    det.check_edges()
    det.draw(path=None)
    two = det.tri_otsu(rgb, keep_tbd=0)
    assert not np.any(two == N.OTHER) and np.array_equal(two, N.classify(rgb, keep_tbd=0)[0])
    # the single-frame entry point with default parameters
    out = np.zeros((h, w), np.uint8)
    assert L.ck_cat_tri_otsu(hd, rgb.ctypes.data, w, h, out.ctypes.data) == 0 and np.array_equal(out, want)


def test_refusals_leave_a_working_handle(det, scene):
    from chalkydri_amd.cat import tri_otsu_params
    L, hd = det._L, det._det._h
    w, h, n = 37, 21, 2
    frames = np.stack([_frame("tags", w, h, 3, i, scene) for i in range(n)])
    cls = np.zeros((n, h, w), np.uint8)
    ok = tri_otsu_params()

    def call(h_=hd, p=C.byref(ok), px=frames.ctypes.data, n_=n, w_=w, ht=h, out=cls.ctypes.data):
        return L.ck_cat_tri_otsu_batch(h_, p, px, n_, w_, ht, out, None, None)

    def still_works():
        cls[:] = 9
        assert call() == 0 and S.mismatches(frames, (cls,) + det.tri_otsu_batch(frames)[1:], {}) == 0

    still_works()
    bad = [dict(h_=None), dict(p=None), dict(px=None), dict(out=None), dict(n_=-1), dict(w_=0), dict(ht=0), dict(w_=-5),
           dict(w_=1 << 16, ht=1 << 15), dict(w_=(1 << 31) - 1, ht=(1 << 31) - 1)]
    for field, vals in (("max_iters", (0, 33)), ("min_delta", (0, 256)), ("keep_tbd", (2,)), ("channels", (2, 0))):
        bad += [dict(p=C.byref(tri_otsu_params(**{field: v}))) for v in vals]
    for kw in bad:
        assert call(**kw) == A.CK_EINVAL, kw
        still_works()
    assert L.ck_cat_tri_otsu(None, frames.ctypes.data, w, h, cls.ctypes.data) == A.CK_EINVAL
    assert L.ck_cat_tri_otsu(hd, None, w, h, cls.ctypes.data) == A.CK_EINVAL
    assert L.ck_cat_tri_otsu(hd, frames.ctypes.data, w, h, None) == A.CK_EINVAL
    assert call(n_=0) == 0                                           # an empty batch is not an error
    still_works()


def test_a_helping_of_the_stress_script(built):
    out = S.run(40, 7)
    assert out["mismatching"] == 0 and out["device_pointer_cases"] > 0, out


def test_the_file_passes_on_the_diagnostics_library_with_poisoned_allocations(built):
    """CK_POISON=1 fills every device allocation with 0xA5: the histogram is zeroed by the call, nothing is read that was not written."""
    if os.environ.get("CK_POISON"):
        pytest.skip("already the poisoned run")
    from conftest import diag_env
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "restatement or neighbours or sentinels or refusals"],
                       env=diag_env(CK_POISON="1"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
