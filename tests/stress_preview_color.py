"""Random colour-preview cases on the device against the numpy restatements (tests/preview_color_ref.py, np_jpeg_enc_color.py):
handle and preview geometry, family, orientation, stride, quality, restart rows, content, overlay on / off, index lists, through
the host, device and ring forms.  usage: stress_preview_color.py N SEED -> one JSON line; the bar is 0 mismatching.  No case is
skipped: an overlay case whose frames hold no tag still compares triples and bytes with an empty mask."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import np_jpeg_enc_color as EC  # noqa: E402
import preview_color_ref as PC  # noqa: E402
import raw_format_ref as R  # noqa: E402


def scene_source(rng, fourcc, frame, o, stride_extra):
    """A raw frame [sh][stride] of `fourcc` whose oriented luma is close to the rendered scene `frame`, with chroma around it."""
    if fourcc in PC.YUV422:
        src = R.pack(R.source_of(frame, o), fourcc, seed=int(rng.integers(1 << 30)))
    else:
        src = R.pack(R.source_of(R.grey_to_rgb(frame, int(rng.integers(1 << 30))), o), fourcc, seed=int(rng.integers(1 << 30)))
    out = np.full((src.shape[0], src.shape[1] + stride_extra), 0x5C, np.uint8)
    out[:, :src.shape[1]] = src
    return out


def run(n_cases, seed):
    import torch
    from chalkydri_amd import scenes
    from chalkydri_amd.detector import AprilTagDetector, IngestRing
    rng = np.random.default_rng(seed)
    bad, frames_total, overlay_cases, empty_overlays, forms = [], 0, 0, 0, {"host": 0, "device": 0, "ring": 0}
    case = 0
    while case < n_cases:
        W, H = int(rng.integers(16, 300)), int(rng.integers(16, 220))
        overlay_handle = bool(rng.random() < 0.3)
        if overlay_handle:
            W, H = (640, 480) if rng.random() < 0.5 else (int(rng.integers(400, 700)), int(rng.integers(300, 500)))
        nb = int(rng.integers(1, 4))
        fourcc = str(rng.choice(PC.FAMILIES))
        o = str(rng.choice(R.ORIENTATIONS))
        form = str(rng.choice(["host", "device", "ring"]))
        sw, sh = R.source_size(W, H, o)
        extra = int(rng.choice([0, 0, 1, 7, 16]))
        stride = R.min_stride(fourcc, sw) + extra
        det = AprilTagDetector(W, H, max_batch=nb)
        if overlay_handle:
            F = scenes.bench_stream(int(rng.integers(0, 1000)), nb, W, H, 4)[0]
            raw = [scene_source(rng, fourcc, f, o, extra) for f in F]
        else:
            raw = [PC.pack_colour(rng, fourcc, sw, sh, stride) for _ in range(nb)]
        ring = dev = None
        if form == "host":
            det.upload_raw(raw, fourcc, o)
            dets = det.detect_batch(None, n=nb) if overlay_handle else None
        elif form == "device":
            off = int(rng.integers(0, 4))
            pitch = stride * sh + int(rng.integers(0, 9))
            dev = torch.zeros(off + pitch * nb, dtype=torch.uint8, device="cuda")
            for i, f in enumerate(raw):
                dev[off + i * pitch:off + i * pitch + stride * sh] = torch.from_numpy(f.reshape(-1)).cuda()
            torch.cuda.synchronize()
            ptr = dev.data_ptr() + off
            if overlay_handle:
                det.upload_raw_device(ptr, nb, stride, pitch, fourcc, o)
                dets = det.detect_batch(None, n=nb)
        else:
            ring = IngestRing(det, 2, fourcc=fourcc, orientation=o)
            slot = int(rng.integers(0, 2))
            for i, f in enumerate(raw):
                ring.write(slot, i, f)
            ring.submit(slot, nb)
            dets = ring.detect(slot, nb)[0] if overlay_handle else None
        for _ in range(int(rng.integers(2, 6))):
            if case >= n_cases:
                break
            width = int(rng.choice([0, 8, W, W + 5, int(rng.integers(8, W + 1))]))
            height = int(rng.choice([0, 8, H, H + 5, int(rng.integers(8, H + 1))]))
            q = int(rng.choice([1, 50, 100, int(rng.integers(1, 101))]))
            rr = int(rng.choice([0, 0, 1, 3, int(rng.integers(1, 9))]))
            ov = bool(overlay_handle and rng.random() < 0.7)
            idx = rng.integers(0, nb, int(rng.integers(1, nb + 1))).tolist()
            pw, ph, _ = EC.layout(width, height, W, H, q, rr)
            kw = dict(width=width, height=height, quality=q, restart_rows=rr, overlay=ov)
            if form == "host":
                tri, files = det.preview_color(idx, **kw), det.preview_jpeg_color(idx, **kw)
            elif form == "device":
                tri = det.preview_color_device(ptr, nb, stride, pitch, fourcc, o, idx, **kw)
                files = det.preview_jpeg_color_device(ptr, nb, stride, pitch, fourcc, o, idx, **kw)
            else:
                tri, files = ring.preview_color(slot, idx, **kw), ring.preview_jpeg_color(slot, idx, **kw)
            forms[form] += 1
            if ov:
                overlay_cases += 1
                empty_overlays += all(len(dets[f]) == 0 for f in idx)
            for k, f in enumerate(idx):
                P = PC.triples_vec(raw[f], fourcc, sw, sh, stride, o, pw, ph, [d.corners() for d in dets[f]] if ov else None)
                ok = np.array_equal(tri[k], P) and files[k] == EC.encode_ycc(P, q, rr)
                frames_total += 1
                if not ok:
                    bad.append({"case": case, "form": form, "fourcc": fourcc, "o": o, "W": W, "H": H, "pw": pw, "ph": ph, "q": q, "rr": rr,
                                "overlay": ov, "frame": f, "triples_equal": bool(np.array_equal(tri[k], P))})
            case += 1
        if ring is not None:
            ring.close()
        det.close()
    return {"stress": "preview_color", "cases": n_cases, "seed": seed, "frames": frames_total, "forms": forms, "overlay_cases": overlay_cases,
            "overlay_cases_without_tags": int(empty_overlays), "mismatching": len(bad), "first": bad[:5]}


if __name__ == "__main__":
    print(json.dumps(run(int(sys.argv[1]), int(sys.argv[2]))))
