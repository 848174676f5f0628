"""Child of tests/test_gpu_jpeg_edges.py: decodes the batches of one .npz file (per family NAME: b_NAME the streams' bytes one after
the other, o_NAME their offsets, w_NAME the expected luma [n][h][w], s_NAME the expected status words) on whatever build of the
library the environment names, each batch twice on one handle and once more through the colour form, compares byte for byte and
prints the mismatching families and a hash of everything the device returned.
usage: python tests/jpeg_edges_child.py batches.npz"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
import numpy as np


def pack(batches):
    """{family: (streams, expected luma, expected status)} as the arrays of the .npz"""
    data = {}
    for fam, (streams, want, st) in batches.items():
        data["b_" + fam] = np.frombuffer(b"".join(streams), np.uint8)
        data["o_" + fam] = np.cumsum([0] + [len(b) for b in streams])
        data["w_" + fam], data["s_" + fam] = want, np.asarray(st, np.uint32)
    return data


def unpack(z, fam):
    blob, offs = z["b_" + fam].tobytes(), z["o_" + fam]
    return [blob[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)], z["w_" + fam], [int(x) for x in z["s_" + fam]]


def run_family(streams, want, want_st, hh=None):
    """What differs from the expected bytes and words: (call, frame, what) for ck_jpeg_luma_batch twice on one handle (the second
    call reuses the workspace of a batch that may hold failed frames) and the luma ck_upload_jpeg_color stages."""
    from chalkydri_amd.detector import AprilTagDetector
    n, h, w = want.shape
    det = AprilTagDetector(w, h, max_batch=n)
    bad = []
    for call in ("first", "second", "color"):
        if call == "color":
            k, st = det.upload_jpeg(streams, return_status=True, color=True)
            got = det.quad_image(None, n) if k == n else np.zeros((0, h, w), np.uint8)
        else:
            got, st = det.decode_jpeg(streams, return_status=True)
        if hh is not None:
            hh.update(np.ascontiguousarray(got).tobytes()); hh.update(np.asarray(st, np.uint32).tobytes())
        if got.shape != want.shape:
            bad.append((call, -1, "shape"))
            continue
        for i in range(n):
            if st[i] != want_st[i]:
                bad.append((call, i, "status %d, expected %d" % (st[i], want_st[i])))
            elif not np.array_equal(got[i], want[i]):
                bad.append((call, i, "%d pixels differ" % int((got[i] != want[i]).sum())))
    det.close()
    return bad


def run(path):
    z = np.load(path)
    bad, hh = 0, hashlib.sha256()
    for fam in sorted(k[2:] for k in z.files if k.startswith("b_")):
        frames_bad = run_family(*unpack(z, fam), hh)
        if frames_bad:
            bad += 1
            print("MISMATCH", fam, frames_bad[:8])
    print("MISMATCHING_FAMILIES", bad)
    print("HASH", hh.hexdigest())
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(sys.argv[1]) else 0)
