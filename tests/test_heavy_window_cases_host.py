"""The cases of tests/test_gpu_heavy_windows.py are not vacuous, and the bounds k_chunk's window step leans on hold: with the oracle
alone (no GPU).  Every frame of tests/heavy_window_cases.py is one cluster that becomes one quad, of 240 points and more (windows of
2 * 20 + 1 = 41 points), and reaches the pinned largest point weight and largest window weight sum — on a numpy restatement of the
oracle's sort and weight formula, which is itself checked against the oracle's count of points after duplicate removal.  The bases
put the middle of the heaviest window on the three wave boundaries of the loaded span and on a span's first position.

Measured when the cases were written (default settings):

  frame      points  ksz  maxima  largest weight  largest window sum  middle of that window
  axis         1200   20       4             361               10811                    130
  diagonal     1692   20     570             361               14801 (= 41 * 361)       443
  shallow      1336   20      85             361               11861                    508

The bounds: k_chunk reads 1 / W from a table of INV_N = 41 * 362 + 1 entries without a branch, so a window's weight sum has to stay
below INV_N whatever the positions hold, and its windows reach 21 positions down and 20 up from the positions it evaluates, which
have to lie inside the KL loaded ones; the constants are read from the sources."""
import math
import os
import re

import numpy as np
import pytest

import heavy_window_cases as hw
import span_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sources():
    src = open(os.path.join(ROOT, "chalkydri_amd", "csrc", "k_chunk.hip")).read()
    hdr = open(os.path.join(ROOT, "chalkydri_amd", "csrc", "ck_internal.h")).read()
    return src, hdr


def test_window_bounds_hold_for_the_sources_constants():
    src, hdr = _sources()
    span = int(re.search(r"constexpr int CK_SPAN = (\d+);", hdr).group(1))
    kl, koff = (int(v) for v in re.search(r"constexpr int KL = (\d+), KOFF = (\d+);", src).groups())
    m = re.search(r"constexpr int INV_N = (\d+) \* (\d+) \+ 1;", src)
    window, ceiling = int(m.group(1)), int(m.group(2))
    ksz_max = int(re.search(r"sKsz\[j\] = \(uint8_t\)\(k > (\d+)u \? \1u : k\);", src).group(1))
    # the weight ceiling is the formula's: isqrt(gx^2 + gy^2) + 1 of two differences of bytes (k_weight_image, oracle/detector.c)
    assert math.isqrt(2 * 255 * 255) + 1 <= ceiling == hw.WEIGHT_CEILING
    assert window == 2 * ksz_max + 1 == hw.WINDOW
    # every window's weight sum is an index into the table, whatever the positions hold (a weight is gathered or 1); the kernel
    # clamps the index all the same
    assert src.count("g_inv_table.v[") == 1 and "g_inv_table.v[min(mw, (uint32_t)(INV_N - 1))]" in src
    # the positions step 3 evaluates, [KOFF - 4, KOFF + CK_SPAN + 4), and their windows' ends lie inside the loaded ones
    assert koff - 4 - ksz_max - 1 >= 0 and koff + span + 3 + ksz_max < kl
    # a span's running sums: the 32-bit ones (W, Mx, My) of all KL loaded positions stay below 2^32, the 64-bit ones below 2^52
    coord = 8192
    assert kl * ceiling * coord < 1 << 32 and kl * ceiling * coord * coord < 1 << 52
    assert (span, koff) == (sc.SPAN, sc.KOFF) and sc.KOFF + sc.SPAN <= kl


@pytest.fixture(scope="module")
def checked(oracle):
    return hw.check(oracle)


def test_frames_reach_their_pinned_weights(checked):
    """One cluster, one quad, windows of 41 points, the pinned largest weight and largest window sum (check asserts them)."""
    fig, quads = checked
    print(fig)
    assert set(fig) == {"axis", "diagonal", "shallow"} and all(len(q) == 1 for q in quads)
    f = hw.frames()
    assert f.shape[1] <= 480 and f.shape[2] <= 640 and set(np.unique(f)) == {0, 255}
    assert all(v[0] >= 240 and v[1] == 20 for v in fig.values())
    # the top of the range: a window of 41 points of the largest weight the formula gives
    assert max(v[3] for v in fig.values()) == math.isqrt(2 * 255 * 255) + 1 == 361
    assert max(v[4] for v in fig.values()) == 41 * 361
    assert all(v[4] >= 41 * 256 for v in fig.values())   # every frame: more than a window of axis-parallel full-contrast points


def test_restated_weights_are_the_oracles_on_a_flat_edge():
    """point_weights on a hand-made edge: 256 beside a vertical 0 | 255 edge, 1 on the rim and on flat ground."""
    im = np.zeros((8, 8), np.uint8)
    im[:, 4:] = 255
    x, y = np.array([7, 5, 3, 0, 7]), np.array([6, 6, 6, 6, 0])   # pixels 4 and 3 straddle the edge, 2 is flat, column 0 and row 0 are rim
    assert hw.point_weights(im, x, y).tolist() == [256, 256, 1, 1, 1]


def test_bases_put_the_heaviest_window_on_the_wave_and_span_boundaries():
    for name, v in hw.PINNED.items():
        mid = v[5]
        bs = hw.bases(mid)
        assert len(bs) == 4 and len(set(bs)) == 4
        at = [(b + sc.EXT_PRE + mid) % sc.SPAN + sc.KOFF for b in bs[:3]]   # where the span that decides it holds it
        assert at == [256, 512, 768], (name, at)
        assert (bs[3] + sc.EXT_PRE + mid) % sc.SPAN == 0                    # the window straddles two spans
        assert all(0 <= b <= sc.BASE_MAX for b in bs)
