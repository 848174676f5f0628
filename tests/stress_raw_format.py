"""Random raw-format cases against the numpy restatement (tests/raw_format_ref.py):  python tests/stress_raw_format.py N SEED
Every case draws an oriented size 16..900 (odd sizes included), a fourcc, an orientation, a row stride at or above the minimum,
a base offset 0..15 bytes and a batch of 1..8 frames, and compares ck_raw_luma_batch byte for byte; every fourth case goes
through device memory (ck_upload_raw_device on a torch tensor with that stride and offset) instead.  One JSON line."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import raw_format_ref as R  # noqa: E402


def make_sources(rng, fourcc, sw, sh, n, stride, off):
    """n source frames in one byte buffer each, `off` bytes into it; returns (views [rows][stride], expected source lumas)."""
    views = []
    for i in range(n):
        img = rng.integers(0, 256, (sh, sw, 3) if R.is_colour(fourcc) else (sh, sw), dtype=np.uint8)
        packed = R.pack(img, fourcc, stride, pad_byte=int(rng.integers(0, 256)), seed=int(rng.integers(1 << 30)))
        raw = np.full(packed.size + off + 16, 0x3C, np.uint8)
        raw[off:off + packed.size] = packed.reshape(-1)
        views.append(raw[off:off + packed.size].reshape(packed.shape))
    return views


def run(n_cases, seed, verbose=False):
    import torch
    from chalkydri_amd.detector import AprilTagDetector
    rng = np.random.default_rng(seed)
    mismatching, device_cases, pixels = [], 0, 0
    dets = {}
    for case in range(n_cases):
        W, H = int(rng.integers(16, 901)), int(rng.integers(16, 901))
        fourcc = R.FOURCCS[int(rng.integers(len(R.FOURCCS)))]
        o = R.ORIENTATIONS[int(rng.integers(4))]
        n = int(rng.integers(1, 9))
        sw, sh = R.source_size(W, H, o)
        stride = R.min_stride(fourcc, sw) + int(rng.choice([0, 0, 1, 3, 5, 16, 24, 37]))
        off = int(rng.integers(0, 16))
        det = dets.get((W, H))
        if det is None:
            if len(dets) >= 8:
                for d in dets.values():
                    d.close()
                dets.clear()
            det = dets[(W, H)] = AprilTagDetector(W, H, max_batch=8)
        views = make_sources(rng, fourcc, sw, sh, n, stride, off)
        want = np.stack([R.expected(v, fourcc, sw, sh, stride, o) for v in views])
        if case % 4 == 3:
            device_cases += 1
            rows = views[0].shape[0]
            pitch = rows * stride + int(rng.integers(0, 9))
            host = np.full(off + n * pitch + 16, 0x3C, np.uint8)
            for i, v in enumerate(views):
                host[off + i * pitch: off + i * pitch + v.size] = v.reshape(-1)
            dev = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            det.upload_raw_device(dev.data_ptr() + off, n, stride, pitch, fourcc, o)
            got = staged(det, n)
        else:
            got = det.raw_luma(views, fourcc, o)
        pixels += want.size
        bad = int((got != want).sum())
        if bad:
            mismatching.append({"case": case, "W": W, "H": H, "fourcc": fourcc, "orientation": o, "n": n, "stride": stride, "off": off,
                                "device": case % 4 == 3, "bytes": bad})
        if verbose:
            print(case, W, H, fourcc, o, n, stride, off, bad, flush=True)
    for d in dets.values():
        d.close()
    return {"cases": n_cases, "seed": seed, "device_cases": device_cases, "pixels": pixels, "mismatching": len(mismatching),
            "first": mismatching[:5]}


def staged(det, n):
    """The handle's staged frames as [n][H][W]: at quad_decimate 1 without a filter the quad image IS the staged frame."""
    assert det.cfg.quad_decimate == 1 and not det.quad_sigma
    return det.quad_image(None, n=n)


if __name__ == "__main__":
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    out = run(n_cases, seed, verbose=len(sys.argv) > 3)
    print(json.dumps(out))
    sys.exit(1 if out["mismatching"] else 0)
