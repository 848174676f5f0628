"""Stress of the coloured-piece detector: `python tests/stress_blobs.py N seed` draws N random cases — geometry, colour family,
orientation, stride and pitch, classes, morphology, capacities — puts the raw frames into device memory and checks
ck_detect_blobs_device against the host twin on ck_blob_rgb_device's pixels, byte for byte, and the masks at both stages.  Run by hand,
and with a small N by tests/test_gpu_blobs.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preview_color_ref as PC  # noqa: E402
import raw_format_ref as R  # noqa: E402

ORIENTATIONS = ("none", "clockwise", "rotate-180", "counterclockwise")


def blocky(rng, sh, ms, bpp):
    """A source frame whose colours come in patches (so that components have size) with noise on top."""
    cell = int(rng.integers(2, 9))
    pal = rng.integers(0, 256, (int(rng.integers(2, 7)), bpp), dtype=np.uint8)
    px = ms // bpp
    pick = np.kron(rng.integers(0, len(pal), ((sh + cell - 1) // cell, (px + cell - 1) // cell)), np.ones((cell, cell), int))[:sh, :px]
    out = np.zeros((sh, ms), np.uint8)
    out[:, :px * bpp] = pal[pick].reshape(sh, px * bpp)
    noise = rng.random((sh, ms)) < rng.choice([0.0, 0.02, 0.2])
    out[noise] = rng.integers(0, 256, int(noise.sum()), dtype=np.uint8)
    return out


def one_case(rng, torch, B, make_detector):
    W, H = int(rng.integers(16, 141)), int(rng.integers(16, 100))
    fourcc, o = str(rng.choice(PC.FAMILIES)), str(rng.choice(ORIENTATIONS))
    n_frames, n = int(rng.integers(1, 4)), int(rng.integers(1, 5))
    sw, sh = R.source_size(W, H, o)
    ms = R.min_stride(fourcc, sw)
    stride = ms + int(rng.choice([0, 1, 5, 16]))
    pitch = stride * sh + int(rng.choice([0, 3, 64]))
    bpp = 2 if fourcc in PC.YUV422 else R.RGB_ORDER[fourcc][0]
    dev = torch.full((3 + pitch * n_frames,), 0x5A, dtype=torch.uint8, device="cuda")
    for i in range(n_frames):
        f = np.full((sh, stride), 0xA7, np.uint8)
        f[:, :ms] = blocky(rng, sh, ms, bpp)
        dev[3 + i * pitch:3 + i * pitch + stride * sh] = torch.from_numpy(f.reshape(-1)).cuda()
    torch.cuda.synchronize()
    src = (dev.data_ptr() + 3, n_frames, stride, pitch, fourcc, o)
    idx = rng.integers(0, n_frames, n)
    classes = []
    for _ in range(int(rng.integers(1, 5))):
        lo, hi = sorted(int(v) for v in rng.integers(0, 256, 2))
        classes.append(B.ColorClass(h_min=int(rng.integers(0, 180)), h_max=int(rng.integers(0, 180)), s_min=int(rng.integers(0, 128)),
                                    s_max=int(rng.integers(128, 256)), v_min=lo // 2, v_max=min(255, hi + 64),
                                    min_area=int(rng.choice([0, 1, 2, 9, 40])), max_area=int(rng.choice([0, 0, 200])),
                                    min_fill_permille=int(rng.choice([0, 300, 900])), min_aspect_permille=int(rng.choice([0, 500])),
                                    max_aspect_permille=int(rng.choice([0, 2000])), ground_z=float(rng.choice([0.0, 0.1]))))
    from chalkydri_amd.camera import make_camera
    cam = make_camera("EUCM", 0.8 * W + 5, 0.8 * W + 6, W / 2.0, H / 2.0, 0.6, 1.1) if rng.random() < 0.5 else None
    a = np.radians(25.0)
    mount = ([0.0, 0.5 * np.cos(a), 0.5 * np.sin(a)], [0.5 * (np.cos(a / 2) + np.sin(a / 2)), -0.5 * (np.cos(a / 2) + np.sin(a / 2)),
             0.5 * (np.cos(a / 2) - np.sin(a / 2)), -0.5 * (np.cos(a / 2) - np.sin(a / 2))]) if cam is not None and rng.random() < 0.7 else None
    pp = B.blob_params(classes, erode=int(rng.integers(0, 5)) if rng.random() < 0.5 else 0, dilate=int(rng.integers(0, 5)) if rng.random() < 0.5 else 0,
                       max_targets=int(rng.choice([0, 1, 4, 16])), max_components=int(rng.choice([1, 3, 64, 4096])), camera=cam,
                       robot_to_cam=mount, max_range=float(rng.choice([2.0, 20.0])))
    cap = int(rng.choice([0, 2, 16]))
    det = make_detector(W, H, 4)
    try:
        rgb = det.blob_rgb(idx, device=src)
        got = det.detect_blobs_device(pp, *src, frames=idx, cap=cap)
        want = B.blobs_host(pp, rgb, cap)
        what = (W, H, fourcc, o, stride - ms, n_frames, list(idx), len(classes), pp.erode, pp.dilate, pp.max_targets, pp.max_components, cap)
        for g, w, name in zip(got, want, ("records", "counts", "status")):
            assert g.tobytes() == w.tobytes(), (name, what)
        c = int(rng.integers(0, len(classes)))
        for stage in (0, 1):
            assert np.array_equal(det.blob_mask(pp, c, stage, idx, device=src), B.mask_host(pp, rgb, c, stage)), ("mask", stage, what)
        return int(want[1].sum()), int(want[2].max())
    finally:
        det.close()


def run(N, seed=0):
    import torch
    from chalkydri_amd import blobs as B
    from chalkydri_amd.detector import AprilTagDetector
    rng = np.random.default_rng(seed)
    targets, flagged = 0, 0
    for _ in range(N):
        t, s = one_case(rng, torch, B, lambda w, h, nb: AprilTagDetector(w, h, max_batch=nb))
        targets += t
        flagged += s != 0
    return targets, flagged


if __name__ == "__main__":
    N, seed = int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 0
    t, f = run(N, seed)
    print(f"stress_blobs ok: {N} cases, {t} targets, {f} cases with a status flag")
