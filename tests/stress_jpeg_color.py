"""Random colour previews of MJPEG frames on the device against the numpy restatement (tests/np_jpeg_color.py) and Pillow's
encoder: stream geometry, sampling, restart interval, quality, orientation, batch, preview size, quality and restart rows of the
preview, index lists, through ck_upload_jpeg_color and through a ring of ck_ingest_create_jpeg_color; a bad stream now and then.
usage: stress_jpeg_color.py N SEED -> one JSON line; the bar is 0 mismatching.  No case is skipped."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import np_jpeg as J  # noqa: E402
import np_jpeg_color as JC  # noqa: E402
import np_jpeg_enc_color as EC  # noqa: E402
import raw_format_ref as R  # noqa: E402

SAMPLINGS = ("444", "422", "440", "420", "grey")


def random_stream(rng, sw, sh):
    """(bytes, C, status) for an sw x sh handle geometry: mostly a good stream, sometimes truncated or of another size."""
    yy, xx = np.mgrid[0:sh, 0:sw]
    luma = np.clip(rng.uniform(-3, 3) * xx + rng.uniform(-3, 3) * yy + rng.uniform(0, 255) + rng.normal(0, rng.choice([3, 30]), (sh, sw)), 0, 255)
    sampling = str(rng.choice(SAMPLINGS))
    chroma = None
    if sampling != "grey":
        chroma = tuple(rng.integers(0, 256, (sh, sw), dtype=np.uint8) if rng.random() < 0.5 else
                       np.clip(luma[::-1] * rng.uniform(0.3, 1) + rng.normal(0, 10, (sh, sw)), 0, 255).astype(np.uint8) for _ in range(2))
    ri = int(rng.choice([0, 0, 1, 2, 7, -1]))
    b = J.encode(luma.astype(np.uint8), sampling, quality=int(rng.integers(20, 99)), restart_interval=abs(ri), restart_rows=ri < 0, chroma=chroma)
    kind = rng.random()
    if kind < 0.05:
        b = b[:int(len(b) * rng.uniform(0.5, 0.9))]
    elif kind < 0.08:
        b = J.encode(luma.astype(np.uint8)[:sh - 1], sampling, chroma=None if chroma is None else tuple(c[:sh - 1] for c in chroma))
    Cc, st = JC.decode_color(b, (sw, sh))
    return b, Cc, st, sampling


def run(n_cases, seed):
    from chalkydri_amd.detector import AprilTagDetector, IngestRing
    rng = np.random.default_rng(seed)
    bad, frames_total, forms, samplings, failed = [], 0, {"host": 0, "ring": 0}, {s: 0 for s in SAMPLINGS}, 0
    case = 0
    while case < n_cases:
        W, H = int(rng.integers(16, 120)), int(rng.integers(16, 100))
        nb = int(rng.integers(1, 5))
        o = str(rng.choice(R.ORIENTATIONS))
        sw, sh = R.source_size(W, H, o)
        form = str(rng.choice(["host", "ring"]))
        det = AprilTagDetector(W, H, max_batch=nb)
        ring = IngestRing(det, 2, fourcc="MJPG", orientation=o, max_frame_bytes=1 << 18, color=True) if form == "ring" else None
        for _ in range(int(rng.integers(1, 4))):       # several uploads on one handle: the workspace grows and is reused
            if case >= n_cases:
                break
            n = int(rng.integers(1, nb + 1))
            S = [random_stream(rng, sw, sh) for _ in range(n)]
            for s in S:
                samplings[s[3]] += 1
                failed += s[2] != 0
            if ring is None:
                _, st = det.upload_jpeg([s[0] for s in S], o, return_status=True, color=True)
                luma = det.quad_image(None, n)
            else:
                slot = int(rng.integers(0, 2))
                for i, s in enumerate(S):
                    ring.write(slot, i, s[0])
                ring.submit(slot, n)
                st = ring.jpeg_status(slot, n)
                luma = None
            status_ok = list(st) == [s[2] for s in S]
            for _ in range(int(rng.integers(1, 4))):
                if case >= n_cases:
                    break
                width = int(rng.choice([0, 8, W, W + 5, int(rng.integers(8, W + 1))]))
                height = int(rng.choice([0, 8, H, H + 5, int(rng.integers(8, H + 1))]))
                q = int(rng.choice([1, 50, 100, int(rng.integers(1, 101))]))
                rr = int(rng.choice([0, 0, 1, 3]))
                idx = rng.integers(0, n, int(rng.integers(1, n + 1))).tolist()
                pw, ph, _ = EC.layout(width, height, W, H, q, rr)
                kw = dict(width=width, height=height, quality=q, restart_rows=rr)
                if ring is None:
                    tri, files = det.preview_color(idx, **kw), det.preview_jpeg_color(idx, **kw)
                else:
                    tri, files = ring.preview_color(slot, idx, **kw), ring.preview_jpeg_color(slot, idx, **kw)
                forms[form] += 1
                for k, f in enumerate(idx):
                    P = JC.preview_triples(S[f][1], o, pw, ph)
                    luma_ok = luma is None or np.array_equal(luma[f], R.orient_vec(S[f][1][..., 0], o))
                    ok = status_ok and luma_ok and np.array_equal(tri[k], P) and files[k] == JC.pillow_file(P, q, rr)
                    frames_total += 1
                    if not ok:
                        bad.append({"case": case, "form": form, "o": o, "W": W, "H": H, "sampling": S[f][3], "pw": pw, "ph": ph, "q": q, "rr": rr,
                                    "frame": f, "status_ok": status_ok, "luma_ok": bool(luma_ok), "triples_equal": bool(np.array_equal(tri[k], P))})
                case += 1
            if ring is not None:
                ring.detect(slot, n)                    # the slot is processed: it may be written again
        if ring is not None:
            ring.close()
        det.close()
    return {"stress": "jpeg_color", "cases": n_cases, "seed": seed, "frames": frames_total, "forms": forms, "samplings": samplings,
            "failed_streams": int(failed), "mismatching": len(bad), "first": bad[:5]}


if __name__ == "__main__":
    print(json.dumps(run(int(sys.argv[1]), int(sys.argv[2]))))
