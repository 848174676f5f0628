"""The colour form of the JPEG decode on the host: tests/np_jpeg_color.py — the restatement the GPU tests compare
against — equals libjpeg-turbo's own YCbCr decode (Pillow's draft("YCbCr")) byte for byte on random streams of every supported
layout, its vectorised upsampler equals the contract's loops, failed and grey frames follow the contract, and the preview's file
reference (Pillow's encoder) equals the repository's numpy encoder."""
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg as J  # noqa: E402
import np_jpeg_color as JC  # noqa: E402
import np_jpeg_enc_color as EC  # noqa: E402

SAMPLINGS = ("444", "422", "440", "420", "grey")


def picture(rng, w, h):
    """Three planes [h][w]: smooth gradients plus noise, so that both low and high frequencies survive the quantiser."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(3):
        a, b, c = rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(0, 255)
        p = a * xx + b * yy + c + rng.normal(0, rng.choice([2, 20, 60]), (h, w))
        out.append(np.clip(p, 0, 255).astype(np.uint8))
    return out


def np_stream(rng, w, h, sampling):
    y, cb, cr = picture(rng, w, h)
    if rng.random() < 0.5:   # full-range chroma
        cb, cr = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    ri = int(rng.choice([0, 0, 1, 2, 3, 5]))
    return J.encode(y, sampling, quality=int(rng.integers(30, 96)), restart_interval=ri, chroma=None if sampling == "grey" else (cb, cr))


def pillow_stream(rng, w, h, subsampling):
    rgb = np.stack(picture(rng, w, h), -1)
    buf = io.BytesIO()
    kw = {"restart_marker_blocks": int(rng.integers(1, 6))} if rng.random() < 0.4 else {}
    Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=int(rng.integers(30, 96)), subsampling=subsampling, **kw)
    return buf.getvalue()


def test_decode_color_equals_libjpeg_on_random_streams():
    """240 streams, none skipped: 30 per Pillow subsampling 0 / 1 / 2 and per np_jpeg.encode sampling (444, 422, 440, 420, grey,
    restart intervals 0 and 1..5 MCUs, random full-range chroma in half of them), widths 17..89 and heights 17..69 (odd sizes and
    sizes that are no multiple of the MCU among them), quality 30..95."""
    rng = np.random.default_rng(20240)
    bad, n, ragged = [], 0, 0
    for k in range(30):
        for kind in ("p0", "p1", "p2") + SAMPLINGS:
            w, h = int(rng.integers(17, 90)), int(rng.integers(17, 70))
            s = pillow_stream(rng, w, h, int(kind[1])) if kind[0] == "p" else np_stream(rng, w, h, kind)
            C, st = JC.decode_color(s)
            want = JC.pillow_ycc(s)
            n += 1
            ragged += (w % 16 != 0) and (h % 16 != 0)
            if st != J.OK or C.shape != want.shape or not np.array_equal(C, want):
                bad.append((kind, w, h, st))
    assert n == 240 and ragged > 100
    assert not bad, (len(bad), bad[:10])


def test_luma_of_the_colour_frame_is_the_luma_decode():
    rng = np.random.default_rng(5)
    for sampling in SAMPLINGS:
        s = np_stream(rng, 51, 37, sampling)
        Y, st = J.decode_luma(s)
        C, stc = JC.decode_color(s, (51, 37))
        assert st == stc == J.OK and np.array_equal(C[..., 0], Y)


def test_vectorised_upsampler_equals_the_loops():
    """Every sampling on frames whose plane is odd, even, and cropped (w < hs cw, h < vs ch), extreme values included."""
    rng = np.random.default_rng(6)
    for hs, vs in ((1, 1), (2, 1), (1, 2), (2, 2)):
        for w, h in ((16, 16), (17, 19), (51, 37), (40, 24), (18, 17)):
            cw, ch = -(-w // hs), -(-h // vs)
            for P in (rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.choice(np.array([0, 255], np.uint8), (ch, cw))):
                assert np.array_equal(JC.upsample_vec(P, hs, vs, w, h), JC.upsample(P, hs, vs, w, h)), (hs, vs, w, h)


def test_edges_of_the_contract():
    """x == 0 and x == 2 cw - 1 give the sample itself; the first and the last row take themselves as the missing neighbour."""
    P = np.array([[10, 200, 30], [250, 0, 90]], np.uint8)
    U = JC.upsample(P, 2, 2, 6, 4)
    assert U[0, 0] == 10 and U[0, 5] == 30 and U[3, 0] == 250 and U[3, 5] == 90
    assert U[0, 1] == (3 * (4 * 10) + 4 * 200 + 7) >> 4 and U[1, 0] == (4 * (3 * 10 + 250) + 8) >> 4
    U = JC.upsample(P, 2, 1, 5, 2)   # the x == 2 cw - 1 column is cropped away
    assert U.shape == (2, 5) and U[0, 4] == (3 * 30 + 200 + 1) >> 2


def test_grey_and_failed_frames():
    rng = np.random.default_rng(7)
    good = np_stream(rng, 40, 24, "420")
    C, st = JC.decode_color(np_stream(rng, 40, 24, "grey"), (40, 24))
    assert st == J.OK and (C[..., 1:] == 128).all() and C[..., 0].any()
    prog = bytearray(good)
    prog[prog.index(b"\xff\xc0") + 1] = 0xC2
    for s, want in ((good[:len(good) // 2], J.CORRUPT), (bytes(prog), J.UNSUPPORTED), (np_stream(rng, 24, 40, "420"), J.GEOMETRY)):
        C, st = JC.decode_color(s, (40, 24))
        assert st == want and C.shape == (24, 40, 3)
        assert (C[..., 0] == 0).all() and (C[..., 1:] == 128).all()


def test_pillow_file_equals_the_numpy_encoder():
    """The two references of the preview's files agree: Pillow's save(quality, subsampling=0) of the YCbCr picture and
    np_jpeg_enc_color.encode_ycc, with and without restart rows."""
    rng = np.random.default_rng(8)
    for (pw, ph), q, rr in (((24, 16), 50, 0), ((37, 21), 50, 1), ((51, 37), 85, 2), ((8, 8), 1, 0), ((40, 24), 100, 1)):
        P = rng.integers(0, 256, (ph, pw, 3), dtype=np.uint8)
        assert JC.pillow_file(P, q, rr) == EC.encode_ycc(P, q, rr), (pw, ph, q, rr)


def test_preview_triples_orient_and_scale():
    rng = np.random.default_rng(9)
    C = rng.integers(0, 256, (37, 51, 3), dtype=np.uint8)
    assert np.array_equal(JC.preview_triples(C, "none", 51, 37), C)
    P = JC.preview_triples(C, "clockwise", 37, 51)
    assert P.shape == (51, 37, 3) and np.array_equal(P[5, 7], C[37 - 1 - 7, 5])   # out[y][x] = S[sh-1-x][y]
    P = JC.preview_triples(C, "counterclockwise", 16, 24)
    oy, ox = ((2 * 3 + 1) * 51) // (2 * 24), ((2 * 2 + 1) * 37) // (2 * 16)
    assert np.array_equal(P[3, 2], C[ox, 51 - 1 - oy])                            # out[y][x] = S[x][sw-1-y]
