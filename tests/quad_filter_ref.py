"""numpy restatement of quad_sigma: the image the quad stages run on.

`quad_image` is the vectorised form the GPU tests compare against; `quad_image_loops` is written line by line from the contract
with plain loops, and tests/test_quad_sigma_host.py checks that the two agree."""
import math

import numpy as np


def kernel(sigma):
    """Steps 1-2 and 7: (ksz, u8 weights) of a sigma; ksz = 1 and no weights when the filter is off."""
    s = np.float32(abs(np.float32(sigma)))
    if math.isnan(s) or math.isinf(s):
        raise ValueError("sigma must be finite")
    if s > np.float32(8.0):
        raise ValueError("|sigma| > 8 is unsupported")
    ksz = int(np.float32(4.0) * s)
    if (ksz & 1) == 0:
        ksz += 1
    if ksz <= 1:
        return 1, np.zeros(0, np.uint8)
    dk = []
    for i in range(ksz):
        x = float(i - ksz // 2) / float(s)
        dk.append(math.exp(-0.5 * (x * x)))
    acc = 0.0
    for v in dk:
        acc += v
    return ksz, np.array([int(v / acc * 255) for v in dk], np.uint8)


def decimate(frame, f):
    return np.ascontiguousarray(np.asarray(frame, np.uint8)[: (frame.shape[0] // f) * f: f, : (frame.shape[1] // f) * f: f])


def _pass_rows(x, k):
    """Step 3 along axis 1 of a 2-D u8 array."""
    ksz = len(k)
    h = ksz // 2
    sz = x.shape[1]
    y = x.copy()
    if sz <= ksz:
        return y
    acc = np.zeros((x.shape[0], sz - ksz), np.uint32)   # outputs i = h .. sz - h - 2
    for j in range(ksz):
        acc += np.uint32(k[j]) * x[:, j: j + sz - ksz].astype(np.uint32)
    y[:, h: sz - h - 1] = (acc >> 8).astype(np.uint8)
    return y


def blur(d, k):
    """Step 4: rows, truncated to u8, then columns."""
    b = _pass_rows(d, k)
    return np.ascontiguousarray(_pass_rows(b.T.copy(), k).T)


def quad_image(frame, sigma, f=1):
    """Q of one frame (steps 1-5)."""
    d = decimate(frame, f) if f > 1 else np.ascontiguousarray(frame, np.uint8)
    ksz, k = kernel(sigma)
    if ksz <= 1:
        return d.copy()
    b = blur(d, k)
    if np.float32(sigma) > 0:
        return b
    return np.clip(2 * d.astype(np.int32) - b.astype(np.int32), 0, 255).astype(np.uint8)


def _convolve_loops(x, sz, k, ksz):
    y = [0] * sz
    for i in range(sz):
        y[i] = x[i]
    for i in range(ksz // 2, sz - ksz // 2 - 1):
        acc = 0
        for j in range(ksz):
            acc += int(k[j]) * int(x[i - ksz // 2 + j])
        y[i] = (acc >> 8) & 0xFFFFFFFF
    return y


def quad_image_loops(frame, sigma, f=1):
    """The same, one pixel at a time, as the contract states it."""
    fr = np.asarray(frame, np.uint8)
    qh, qw = fr.shape[0] // f, fr.shape[1] // f
    d = [[int(fr[y * f][x * f]) for x in range(qw)] for y in range(qh)]
    ksz, k = kernel(sigma)
    if ksz <= 1:
        return np.array(d, np.uint8).reshape(qh, qw)
    rows = [_convolve_loops(d[y], qw, k, ksz) for y in range(qh)]
    b = [[0] * qw for _ in range(qh)]
    for x in range(qw):
        col = _convolve_loops([rows[y][x] for y in range(qh)], qh, k, ksz)
        for y in range(qh):
            b[y][x] = col[y]
    q = [[0] * qw for _ in range(qh)]
    for y in range(qh):
        for x in range(qw):
            if np.float32(sigma) > 0:
                q[y][x] = b[y][x]
            else:
                q[y][x] = min(255, max(0, 2 * d[y][x] - b[y][x]))
    return np.array(q, np.uint8).reshape(qh, qw)
