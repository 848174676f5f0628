"""quad_sigma on the host (no device): the library's weights equal the restatement of the contract for every sigma it accepts and
refuse what it does not; the vectorised restatement the GPU tests compare against equals the loop version written line by line
from the contract; the C++ layer exposes the new setter."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import quad_filter_ref as R
from chalkydri_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from chalkydri_amd.detector import _bind
    from chalkydri_amd._lib import lib
    return _bind(lib())


def _kernel(L, sigma, cap=33):
    k = (C.c_uint8 * 64)()
    n = C.c_int32(-7)
    rc = L.ck_quad_sigma_kernel(sigma, k, cap, C.byref(n))
    return rc, n.value, np.array(k[:max(n.value, 0)], np.uint8)


def _sigmas():
    grid = [i / 100.0 for i in range(-800, 801)]
    return grid + [0.4999, 0.5, -0.5, 1e-30, -0.0]


def test_weights_equal_the_restatement(built):
    L = _lib()
    classes = set()
    for s in _sigmas():
        rc, ksz, k = _kernel(L, s)
        want_ksz, want_k = R.kernel(float(np.float32(s)))
        assert rc == A.CK_OK, s
        assert ksz == want_ksz, (s, ksz, want_ksz)
        if ksz > 1:
            assert np.array_equal(k, want_k), (s, k, want_k)
            assert int(k.sum()) < 256
            classes.add(0 if ksz <= 5 else 1 if ksz <= 9 else 2 if ksz <= 17 else 3)
    assert classes == {0, 1, 2, 3}
    assert _kernel(L, 0.4999)[1] == 1 and _kernel(L, 0.5)[1] == 3 and _kernel(L, -0.0)[1] == 1 and _kernel(L, 8.0)[1] == 33


def test_weights_refuse_what_the_kernel_cannot_run(built):
    L = _lib()
    above8 = float(np.nextafter(np.float32(8.0), np.float32(9.0)))
    assert _kernel(L, float("nan"))[0] == A.CK_EINVAL
    assert _kernel(L, float("inf"))[0] == A.CK_EINVAL
    assert _kernel(L, float("-inf"))[0] == A.CK_EINVAL
    assert _kernel(L, above8)[0] == A.CK_EUNSUPPORTED
    assert _kernel(L, -above8)[0] == A.CK_EUNSUPPORTED
    assert _kernel(L, 8.5)[0] == A.CK_EUNSUPPORTED
    k = (C.c_uint8 * 64)()
    n = C.c_int32(0)
    assert L.ck_quad_sigma_kernel(1.0, k, 33, None) == A.CK_EINVAL          # no place for ksz
    assert L.ck_quad_sigma_kernel(1.0, None, 33, C.byref(n)) == A.CK_EINVAL  # no place for the weights
    assert L.ck_quad_sigma_kernel(0.2, None, 0, C.byref(n)) == A.CK_OK and n.value == 1   # off: no weights needed
    rc, ksz, _ = _kernel(L, 3.0, cap=12)                                     # 13 taps do not fit 12
    assert rc == A.CK_EINVAL and ksz == 13
    assert _kernel(L, 3.0, cap=13)[0] == A.CK_OK


@pytest.mark.parametrize("sigma", [0.8, 1.6, 3.0, 6.0, -0.8, -1.5, -4.0, 8.0])
def test_vectorised_restatement_equals_the_loops(sigma):
    ksz = R.kernel(sigma)[0]
    rng = np.random.default_rng(int(abs(sigma) * 100) + (sigma < 0))
    sizes = sorted({1, 2, 3, ksz - 1, ksz, ksz + 1, ksz + 2, ksz + 3} - {0})
    for hh in sizes:
        for ww in (1, ksz, ksz + 3):
            fr = rng.integers(0, 256, (hh, ww), dtype=np.uint8)
            assert np.array_equal(R.quad_image(fr, sigma), R.quad_image_loops(fr, sigma)), (hh, ww)
    fr = rng.integers(0, 256, (2 * ksz + 7, 2 * ksz + 5), dtype=np.uint8)
    assert np.array_equal(R.quad_image(fr, sigma, 2), R.quad_image_loops(fr, sigma, 2))


def test_restatement_behaves_like_a_blur_and_a_sharpen():
    rng = np.random.default_rng(3)
    fr = rng.integers(0, 256, (40, 50), dtype=np.uint8)
    assert np.array_equal(R.quad_image(fr, 0.3), fr) and np.array_equal(R.quad_image(fr, -0.49), fr)
    b = R.quad_image(fr, 2.0).astype(float)
    s = R.quad_image(fr, -2.0).astype(float)
    inner = (slice(8, -9), slice(8, -9))
    assert b[inner].std() < 0.5 * fr[inner].std() < s[inner].std()
    assert np.array_equal(R.quad_image(fr, 2.0)[:4, :4], fr[:4, :4])   # copied by both passes (h = 4)


def test_cpp_layer_exposes_quad_sigma(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text('#include "chalkydri.hpp"\n'
                   "void f(chalkydri::Handle &h) { h.set_quad_sigma(0.8f); }\n"
                   "float g() { chalkydri::AprilTags::Config c; c.quad_sigma = -0.8f; return c.quad_sigma; }\n"
                   "int k(uint8_t *w, int32_t *n) { return ck_quad_sigma_kernel(1.0f, w, 33, n); }\n"
                   "int q(ck_handle_t *h, uint8_t *o) { return ck_quad_image_batch(h, nullptr, 1, o) + ck_set_quad_sigma(h, 1.0f); }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
