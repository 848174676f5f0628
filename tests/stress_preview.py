"""Random preview cases on the device against the numpy restatement (tests/np_jpeg_enc.py): handle and preview geometry, quality,
restart rows, content, overlay on / off, index lists.  usage: stress_preview.py N SEED -> one JSON line; the bar is 0 mismatching.
No case is skipped: an overlay case whose frames hold no tag still compares luma and bytes with an empty mask."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import np_jpeg_enc as E  # noqa: E402


def content(rng, kind, h, w):
    if kind == 0:
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    if kind == 1:
        return np.full((h, w), rng.integers(0, 256), np.uint8)
    if kind == 2:
        yy, xx = np.mgrid[0:h, 0:w]
        return ((xx + yy + int(rng.integers(0, 2))) % 2 * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 70 * np.sin(xx / (5.0 + 40 * rng.random())) * np.cos(yy / (5.0 + 40 * rng.random()))
    return np.clip(base + rng.normal(0, 1 + 20 * rng.random(), (h, w)), 0, 255).astype(np.uint8)


def run(n_cases, seed):
    from chalkydri_amd import scenes
    from chalkydri_amd.detector import AprilTagDetector
    rng = np.random.default_rng(seed)
    bad, frames_total, overlay_cases, empty_overlays = [], 0, 0, 0
    case = 0
    while case < n_cases:
        W, H = int(rng.integers(16, 700)), int(rng.integers(16, 520))
        overlay_handle = bool(rng.random() < 0.3)
        if overlay_handle:
            W, H = (640, 480) if rng.random() < 0.5 else (int(rng.integers(400, 800)), int(rng.integers(300, 600)))
        nb = int(rng.integers(1, 5))
        det = AprilTagDetector(W, H, max_batch=nb)
        if overlay_handle:
            F = scenes.bench_stream(int(rng.integers(0, 1000)), nb, W, H, 4)[0]
        else:
            F = np.stack([content(rng, int(rng.integers(0, 4)), H, W) for _ in range(nb)])
        det.upload(F)
        dets = det.detect_batch(None, n=nb) if overlay_handle else None
        for _ in range(int(rng.integers(2, 7))):
            if case >= n_cases:
                break
            width = int(rng.choice([0, 8, W, W + 5, int(rng.integers(8, W + 1))]))
            height = int(rng.choice([0, 8, H, H + 5, int(rng.integers(8, H + 1))]))
            q = int(rng.choice([1, 50, 100, int(rng.integers(1, 101))]))
            rr = int(rng.choice([0, 0, 1, 3, int(rng.integers(1, 9))]))
            ov = bool(overlay_handle and rng.random() < 0.7)
            idx = rng.integers(0, nb, int(rng.integers(1, nb + 1))).tolist()
            pw, ph, _ = E.layout(width, height, W, H, q, rr)
            luma = det.preview_luma(idx, width=width, height=height, quality=q, restart_rows=rr, overlay=ov)
            files = det.preview_jpeg(idx, width=width, height=height, quality=q, restart_rows=rr, overlay=ov)
            if ov:
                overlay_cases += 1
                empty_overlays += all(len(dets[f]) == 0 for f in idx)
            for k, f in enumerate(idx):
                P = E.preview(F[f], pw, ph, [d.corners() for d in dets[f]] if ov else None)
                ok = np.array_equal(luma[k], P) and files[k] == E.encode_grey(P, q, rr)
                frames_total += 1
                if not ok:
                    bad.append({"case": case, "W": W, "H": H, "pw": pw, "ph": ph, "q": q, "rr": rr, "overlay": ov, "frame": f,
                                "luma_equal": bool(np.array_equal(luma[k], P))})
            case += 1
        det.close()
    return {"stress": "preview", "cases": n_cases, "seed": seed, "frames": frames_total, "overlay_cases": overlay_cases,
            "overlay_cases_without_tags": int(empty_overlays), "mismatching": len(bad), "first": bad[:5]}


if __name__ == "__main__":
    print(json.dumps(run(int(sys.argv[1]), int(sys.argv[2]))))
