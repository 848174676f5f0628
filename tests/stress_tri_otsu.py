"""Random tri-class Otsu cases against the restatement (tests/np_tri_otsu.py):  python tests/stress_tri_otsu.py CASES SEED
Every case draws a geometry 1..700 x 1..500, a batch of 1..4 frames of mixed content (flat, two levels, noise of several amplitudes,
ramps, checkers, blurred blobs; grey frames replicated or independent channels), the parameters, the channel count and the kind
of pointers (host arrays, or torch tensors on the device for all four arrays), and compares classes, records and histograms of
ck_cat_tri_otsu_batch byte for byte.  One JSON line."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import np_tri_otsu as N  # noqa: E402


def content(rng, w, h, ch):
    kind = int(rng.integers(0, 7))
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 0:
        g = np.full((h, w), int(rng.integers(0, 256)), np.uint8)
    elif kind == 1:
        a, b = (int(v) for v in rng.integers(0, 256, 2))
        g = np.where(rng.random((h, w)) < rng.uniform(0.05, 0.95), a, b).astype(np.uint8)
    elif kind == 2:
        amp = int(rng.choice([1, 2, 8, 32, 128]))
        g = np.clip(int(rng.integers(0, 256)) + rng.integers(-amp, amp + 1, (h, w)), 0, 255).astype(np.uint8)
    elif kind == 3:
        g = ((xx * int(rng.integers(1, 9)) + yy * int(rng.integers(0, 5))) & 255).astype(np.uint8)
    elif kind == 4:
        cell = int(rng.integers(2, 40))
        g = np.where(((yy // cell) + (xx // cell)) % 2 == 0, int(rng.integers(0, 100)), int(rng.integers(150, 256)))
        g = np.clip(g + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)
    elif kind == 5:                                                 # three populations: dark, bright and a soft middle
        r = np.hypot(xx - w * rng.random(), yy - h * rng.random()) / max(w, h)
        g = np.clip(40 + 180 / (1 + np.exp((r - 0.3) * rng.uniform(5, 60))) + rng.integers(-10, 11, (h, w)), 0, 255).astype(np.uint8)
    else:
        return rng.integers(0, 256, (h, w, ch), dtype=np.uint8)     # independent channels
    if ch == 1:
        return g[..., None]
    return np.clip(np.stack([g] * 3, -1).astype(np.int16) + rng.integers(-2, 3, (h, w, 3)), 0, 255).astype(np.uint8)


def mismatches(frames, got, kw):
    """frames [n][h][w][c]; got = (classes, records, hists) as numpy arrays -> number of frames that differ in any output"""
    cls, infos, hists = got
    bad = 0
    for i in range(len(frames)):
        wc, wi, wh = N.classify(frames[i], **kw)
        ok = cls[i].tobytes() == wc.tobytes() and infos[i].tobytes() == wi.tobytes() and hists[i].tobytes() == wh.tobytes()
        ok = ok and int(infos[i]["n_black"]) + int(infos[i]["n_white"]) + int(infos[i]["n_other"]) == wc.size
        bad += not ok
    return bad


def to_numpy(got):
    from chalkydri_amd.cat import TRI_INFO_DTYPE
    cls, infos, hists = (t.cpu().numpy() for t in got)
    return cls, np.ascontiguousarray(infos).view(TRI_INFO_DTYPE).reshape(-1), hists.view(np.uint32)


def run(n_cases, seed, verbose=False):
    from chalkydri_amd.cat import CatDetector
    rng = np.random.default_rng(seed)
    det = CatDetector(64, 48)                                       # (the call does not use the handle's geometry)
    mismatching, n_frames, on_device = [], 0, 0
    for case in range(n_cases):
        w, h = (int(rng.integers(1, 701)), int(rng.integers(1, 501))) if case % 4 else (int(rng.integers(1, 40)), int(rng.integers(1, 12)))
        n, ch = int(rng.integers(1, 5)), int(rng.choice([1, 3]))
        frames = np.stack([content(rng, w, h, ch) for _ in range(n)])
        kw = {} if case % 3 == 0 else {"max_iters": int(rng.integers(1, 33)), "min_delta": int(rng.integers(1, 5)), "keep_tbd": int(rng.integers(0, 2))}
        device = bool(rng.integers(0, 2))
        if device:
            import torch
            got = to_numpy(det.tri_otsu_batch(torch.from_numpy(frames).cuda(), **kw))
            on_device += 1
        else:
            got = det.tri_otsu_batch(frames, **kw)
        bad = mismatches(frames, got, kw)
        n_frames += n
        if bad:
            mismatching.append({"case": case, "w": w, "h": h, "n": n, "channels": ch, "device": device, "params": kw, "frames": bad})
        if verbose:
            print(case, w, h, n, ch, device, kw, bad, flush=True)
    det.close()
    return {"cases": n_cases, "seed": seed, "frames": n_frames, "device_pointer_cases": on_device, "mismatching": len(mismatching),
            "first": mismatching[:5]}


if __name__ == "__main__":
    out = run(int(sys.argv[1]) if len(sys.argv) > 1 else 100, int(sys.argv[2]) if len(sys.argv) > 2 else 1, verbose=len(sys.argv) > 3)
    print(json.dumps(out))
    sys.exit(1 if out["mismatching"] else 0)
