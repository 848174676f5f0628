"""CPU: the numpy restatement of the preview encoder (tests/np_jpeg_enc.py) equals libjpeg(-turbo) as Pillow drives it, byte for
byte, whole files; its output decodes through the existing restatement of the decoder as Pillow decodes it; ck_preview_layout,
ck_preview_params_default and the multipart framing without a device; the overlay restatement's invariances."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg as J  # noqa: E402
import np_jpeg_enc as E  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

Image = pytest.importorskip("PIL.Image")

SIZES = [(640, 480), (320, 200), (333, 77), (75, 100), (33, 17), (24, 16), (8, 8)]
QUALITIES = [1, 5, 20, 33, 50, 75, 90, 100]


def pillow_has_restart_rows():
    buf0, buf1 = io.BytesIO(), io.BytesIO()
    im = Image.fromarray(np.zeros((32, 32), np.uint8))
    im.save(buf0, "JPEG", quality=50, optimize=False)
    im.save(buf1, "JPEG", quality=50, optimize=False, restart_marker_rows=1)
    return buf0.getvalue() != buf1.getvalue()


def pillow_encode(P, q, rr):
    buf = io.BytesIO()
    kw = {"restart_marker_rows": rr} if rr else {}
    Image.fromarray(P).save(buf, "JPEG", quality=q, optimize=False, **kw)
    return buf.getvalue()


def content(rng, kind, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "flat":
        return np.full((h, w), 97, np.uint8)
    if kind == "ramp":
        return ((xx * 3 + yy * 2) % 256).astype(np.uint8)
    if kind == "smooth":
        return np.clip(128 + 90 * np.sin(xx / 9.0) * np.cos(yy / 13.0) + rng.normal(0, 3, (h, w)), 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    if kind == "zero":
        return np.zeros((h, w), np.uint8)
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    if kind == "checker0":
        return (((xx + yy) % 2) * 255).astype(np.uint8)
    if kind == "checker1":
        return (((xx + yy + 1) % 2) * 255).astype(np.uint8)
    assert kind == "pixel"
    return np.where((xx % 8 == 3) & (yy % 8 == 5), 255, 0).astype(np.uint8)


KINDS = ["flat", "ramp", "smooth", "noise", "zero", "full", "checker0", "checker1", "pixel"]


def test_whole_files_equal_pillow():
    """Whole files byte-equal to Pillow / libjpeg-turbo: 7 sizes (both dimensions = 0 and != 0 mod 8, down to 8 x 8) x 8
    qualities (1, 50 and 100 among them) x restart_rows 0, 1, 3 x content from flat through noise and the extreme blocks."""
    with_rows = pillow_has_restart_rows()
    rng = np.random.default_rng(12)
    cases, bad, self_checked = 0, [], 0
    for w, h in SIZES:
        for qi, q in enumerate(QUALITIES):
            for rr in (0, 1, 3):
                # 3 of the 9 kinds per (size, quality, restart) cell, rotating, so that every kind meets every size and restart value
                for k in range(3):
                    kind = KINDS[(3 * qi + k + rr + SIZES.index((w, h))) % len(KINDS)]
                    P = content(rng, kind, h, w)
                    got = E.encode_grey(P, q, rr)
                    cases += 1
                    if rr and not with_rows:   # this Pillow cannot write restart markers: the restatement's own decode instead
                        self_checked += 1
                        ok = np.array_equal(J.decode_luma(got)[0], J.decode_luma(E.encode_grey(P, q, 0))[0])
                    else:
                        ok = got == pillow_encode(P, q, rr)
                    if not ok:
                        bad.append((w, h, q, rr, kind))
    print(f"{cases} cases, {self_checked} compared against the restatement's own decode (no restart_marker_rows in this Pillow)")
    assert cases >= 300 and not bad, (len(bad), bad[:10])


def test_extreme_blocks_every_quality():
    """The blocks that come closest to the FDCT's 32-bit bound, at every quality 1..100 on a 24 x 16 image."""
    rng = np.random.default_rng(3)
    bad = []
    for kind in ("zero", "full", "checker0", "checker1", "pixel", "noise"):
        P = content(rng, kind, 16, 24)
        for q in range(1, 101):
            if E.encode_grey(P, q, 0) != pillow_encode(P, q, 0):
                bad.append((kind, q))
    assert not bad, bad[:10]


def test_fdct_stays_inside_32_bits():
    """The column pass's intermediates on the extreme blocks stay below 2^31 (k_jpegenc.hip computes them in int)."""
    rng = np.random.default_rng(4)
    blocks = [content(rng, k, 8, 8).astype(np.int64) - 128 for k in KINDS]
    x = 2 * np.arange(8) + 1
    for u in range(8):       # the sign pattern of every DCT basis function at full swing: what maximises that coefficient
        for v in range(8):
            basis = np.cos(x[None, :] * u * np.pi / 16) * np.cos(x[:, None] * v * np.pi / 16)
            blocks += [np.where(basis > 0, 127, -128), np.where(basis > 0, -128, 127)]
    B = np.clip(np.stack(blocks), -128, 127)
    rows = E._fdct_1d(B, True)
    assert np.abs(rows).max() <= 4097
    # the largest sums the pass forms: bounded by the products of the constants with the inputs' sums
    cols = rows.transpose(0, 2, 1)
    t = [cols[..., k] for k in range(8)]
    tmp4, tmp5, tmp6, tmp7 = t[3] - t[4], t[2] - t[5], t[1] - t[6], t[0] - t[7]
    z5 = (tmp4 + tmp6 + tmp5 + tmp7) * 9633
    worst = np.abs(tmp6 * 25172).max() + np.abs((tmp5 + tmp6) * 20995).max() + np.abs((tmp4 + tmp6) * 16069).max() + np.abs(z5).max()
    assert worst + (1 << 14) < 2 ** 31, worst
    assert np.abs(E.fdct_islow(B)).max() < 2 ** 15


def test_decodes_as_pillow_decodes():
    """np_jpeg.decode_luma(encode_grey(P)) equals Pillow's decode of the same bytes: the encoder meets the existing decoder."""
    rng = np.random.default_rng(8)
    for (w, h), q, rr, kind in [((75, 100), 50, 0, "smooth"), ((33, 17), 90, 1, "noise"), ((320, 200), 20, 3, "ramp"),
                                ((24, 16), 100, 1, "checker0"), ((8, 8), 1, 0, "noise")]:
        b = E.encode_grey(content(rng, kind, h, w), q, rr)
        mine, st = J.decode_luma(b)
        assert st == J.OK
        assert np.array_equal(mine, np.asarray(Image.open(io.BytesIO(b)).convert("L"))), (w, h, q, rr, kind)


def test_layout_defaults_and_framing(built):
    from chalkydri_amd.detector import mjpeg_part, preview_layout, preview_params, MjpegStream, _bind
    from chalkydri_amd._lib import ChalkydriError, lib
    L = _bind(lib())
    pp = A.PreviewParams()
    L.ck_preview_params_default(C.byref(pp))
    assert (pp.width, pp.height, pp.quality, pp.restart_rows, pp.overlay) == (640, 480, 50, 0, 0)   # mjpeg.rs:41-49,116
    assert preview_layout(pp, 1280, 800)[:2] == (640, 480)
    assert preview_layout(pp, 272, 200)[:2] == (272, 200)                     # clipped: the library never enlarges
    assert preview_layout(preview_params(0, 0), 641, 479)[:2] == (641, 479)   # 0 = the frame's
    assert preview_layout(preview_params(8, 8), 641, 479)[:2] == (8, 8)
    assert L.ck_preview_layout(C.byref(pp), 640, 480, None, None, None) == A.CK_OK
    assert L.ck_preview_layout(None, 640, 480, None, None, None) == A.CK_EINVAL

    def refused(W=640, H=480, **kw):
        try:
            preview_layout(preview_params(**kw), W, H)
        except ChalkydriError as e:
            return e.code == A.CK_EINVAL
        return False
    for kw in ({"width": 7}, {"height": 7}, {"width": -1}, {"height": -1}, {"quality": 0}, {"quality": 101}, {"restart_rows": -1},
               {"restart_rows": 820}, {"W": 0}, {"H": 0}, {"W": 7}, {"H": 5, "height": 0}):
        assert refused(**kw), kw
    assert not refused(restart_rows=819)                                       # DRI = 819 * 80 = 65520
    # the restatement's layout is the library's, value for value
    for W, H, w, h, q, rr in [(1280, 800, 640, 480, 50, 0), (272, 200, 640, 480, 1, 3), (641, 479, 0, 0, 100, 1), (16, 16, 8, 8, 50, 7)]:
        assert preview_layout(preview_params(w, h, q, rr), W, H) == E.layout(w, h, W, H, q, rr)
    # max_bytes bounds the worst case tried: quality 100 noise, every restart setting
    rng = np.random.default_rng(1)
    for (w, h) in [(640, 480), (33, 17), (8, 8)]:
        for rr in (0, 1):
            P = rng.integers(0, 256, (h, w)).astype(np.uint8)
            assert len(E.encode_grey(P, 100, rr)) <= preview_layout(preview_params(w, h, 100, rr), w, h)[2]
    j = E.encode_grey(np.zeros((8, 8), np.uint8))
    want = b"--frame\r\nContent-Length: " + str(len(j)).encode() + b"\r\nContent-Type: image/jpeg\r\n\r\n" + j
    assert mjpeg_part(j) == want == E.mjpeg_part(j)
    s = MjpegStream(20)
    assert s.part(j, 10.0) == want and s.part(j, 10.04) is None and s.part(j, 10.051) == want   # drop-only, 20 per second


def test_overlay_restatement_invariances():
    W, H, pw, ph = 1280, 800, 640, 480
    P = np.random.default_rng(2).integers(0, 256, (ph, pw)).astype(np.uint8)
    a = np.array([[100.5, 120.25], [400.0, 90.0], [420.75, 380.5], [90.0, 410.0]])
    b = np.array([[700.0, 300.0], [900.0, 310.0], [880.0, 500.0], [690.0, 480.0]])
    far = np.array([[-50.0, -20.0], [1500.0, 30.0], [1400.0, 900.0], [-10.0, 850.0]])          # corners outside the frame
    m = E.overlay_mask([a, b, far], pw, ph, W, H)
    assert m.any() and m.shape == (ph, pw)
    assert np.array_equal(m, E.overlay_mask([far, b[::-1], a[::-1]], pw, ph, W, H))             # winding and order
    assert np.array_equal(m, E.overlay_mask([np.roll(a, 1, axis=0), b, far, a], pw, ph, W, H))  # start corner, a repeated quad
    mf = E.overlay_mask([far], pw, ph, W, H)
    assert [E.corner_pixel(p, pw, ph, W, H) for p in far] == [(0, 0), (pw - 1, 18), (pw - 1, ph - 1), (0, ph - 1)]   # clamped
    assert mf[0, 0] and mf[18, pw - 1] and mf[ph - 1, pw - 1] and mf[ph - 1, 0] and mf[ph - 1, pw // 2]
    assert E.corner_pixel((1279.99, 799.99), pw, ph, W, H) == (639, 479) and E.corner_pixel((0.0, 0.0), pw, ph, W, H) == (0, 0)
    assert np.array_equal(E.apply_overlay(P, E.overlay_mask([], pw, ph, W, H)), P)              # nothing detected: unchanged
    out = E.apply_overlay(P, m)
    assert np.array_equal(out[~m], P[~m]) and np.array_equal(out[m], np.where(P[m] < 128, 255, 0))
    for p0, p1 in [((3, 4), (17, 9)), ((17, 9), (3, 4)), ((5, 5), (5, 5)), ((0, 9), (9, 0)), ((2, 7), (2, 1))]:
        px = E.line_pixels(p0, p1)
        assert set(px) == set(E.line_pixels(p1, p0)) and p0 in px and p1 in px
        assert len(px) == max(abs(p0[0] - p1[0]), abs(p0[1] - p1[1])) + 1
