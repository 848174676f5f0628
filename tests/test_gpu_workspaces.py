"""The on-demand workspaces (JPEG decode, raw staging, preview, exposure; csrc/ck_grow.h) grow by freeing a buffer and allocating
it again.  One handle takes the same calls with 1, then 4, then 1 frames, so every buffer grows once and is then used below its
capacity: each result must be byte-equal to the same call on a handle that only ever saw that count.  A pointer kept across the
growth, a capacity that was not updated, or bytes expected to survive it would show as a difference (with CK_POISON=1 the new
buffer holds 0xA5, not whatever the allocator happened to return).  The same through a JPEG and a raw ingest ring, and the
destructors leave no runtime error behind for the next handle."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg as J  # noqa: E402
import np_tag_render as T  # noqa: E402
import raw_format_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, NB, FAM = 64, 48, 4, "tag16h5"
COUNTS = (1, 4, 1)
ROI = (8, 4, 56, 40)


def frames():
    """NB frames of W x H, one tag each (other ids, places and turns), and their JPEG and YUYV forms."""
    from chalkydri_amd import family
    fam = family(FAM)
    codes = np.ctypeslib.as_array(fam.contents.codes, (fam.contents.ncodes,))
    imgs = []
    for i in range(NB):
        tag = {"fam": fam, "code": int(codes[3 * i + 1]), "corners": T.pose(26 + 4 * i, 22 + i, 26 + i, 90 * i + 7)}
        imgs.append(T.render(W, H, [tag], seed=40 + i, noise=1.0)[0])
    jpegs = [J.encode(f, sampling=("420", "grey", "422", "444")[i], quality=90, restart_interval=(0, 3)[i % 2]) for i, f in enumerate(imgs)]
    yuyv = [R.pack(f, "YUYV", seed=i) for i, f in enumerate(imgs)]
    return np.stack(imgs), jpegs, yuyv


def det_key(dets):
    return [[(d.id(), d.hamming(), d.decision_margin(), d.corners().tobytes(), d.center().tobytes()) for d in f] for f in dets]


def handle_calls(det, n, imgs, jpegs, yuyv):
    """The calls of one count on one handle; every result as bytes (or plain values)."""
    out = []
    det.upload_jpeg(jpegs[:n])
    out.append(det.preview_luma(n=n, width=48, height=40).tobytes())
    det.upload_raw(yuyv[:n], "YUYV")
    luma = det.raw_luma(yuyv[:n], "YUYV")
    assert np.array_equal(luma, imgs[:n])                        # (YUYV carries the luma itself: the staged frames are the frames)
    out.append(luma.tobytes())
    out.append(det.preview_jpeg(n=n, width=48, height=40, quality=50, restart_rows=1))
    dets = det.detect_batch(None, n=n)
    assert all(len(f) >= 1 for f in dets)                        # the overlay has something to draw in every frame
    out.append(det_key(dets))
    out.append(det.preview_jpeg(n=n, width=48, height=40, quality=50, overlay=True))
    out.append(det.exposure_stats(n=n, roi=ROI).tobytes())
    return out


def ring_calls(det, ring, slot, n, data, jpeg):
    """One use of a slot: n frames written, submitted, metered and detected."""
    for i in range(n):
        ring.write(slot, i, data[i])
    ring.submit(slot, n)
    out = [ring.exposure_stats(slot, n=n, roi=ROI).tobytes()]
    dets, status = ring.detect(slot, n)
    assert all(len(f) >= 1 for f in dets)
    out += [det_key(dets), status.tolist()]
    if jpeg:
        out.append(ring.jpeg_status(slot, n))
    return out


def new_detector():
    from chalkydri_amd.detector import AprilTagDetector
    return AprilTagDetector(W, H, max_batch=NB, families=(FAM,), bits_corrected=0)


def test_handle_workspaces_across_growth(built):
    imgs, jpegs, yuyv = frames()
    want = {}
    for n in sorted(set(COUNTS)):
        fresh = new_detector()
        want[n] = handle_calls(fresh, n, imgs, jpegs, yuyv)
        fresh.close()
    det = new_detector()
    for step, n in enumerate(COUNTS):
        got = handle_calls(det, n, imgs, jpegs, yuyv)
        for k, (g, w) in enumerate(zip(got, want[n])):
            assert g == w, (step, n, k)
    det.close()


@pytest.mark.parametrize("code", ["MJPG", "YUYV"])
def test_ring_workspaces_and_teardown(built, code):
    from chalkydri_amd.detector import IngestRing
    imgs, jpegs, yuyv = frames()
    jpeg = code == "MJPG"
    data = jpegs if jpeg else yuyv
    cap = max(len(b) for b in jpegs) if jpeg else 0              # (these small frames compress to more than the default of sw * sh bytes)
    want = {}
    for n in sorted(set(COUNTS)):
        fresh = new_detector()
        ring = IngestRing(fresh, 2, fourcc=code, max_frame_bytes=cap)
        want[n] = ring_calls(fresh, ring, 0, n, data, jpeg)
        ring.close()
        fresh.close()
    for again in range(2):                                       # the second round: both created again after both were destroyed
        det = new_detector()                                     # (raises unless ck_create returns CK_OK)
        ring = IngestRing(det, 2, fourcc=code, max_frame_bytes=cap)
        for step, n in enumerate(COUNTS):
            got = ring_calls(det, ring, step % 2, n, data, jpeg)
            for k, (g, w) in enumerate(zip(got, want[n])):
                assert g == w, (again, step, n, k)
        # a detect call of the handle itself: CK_OK (it raises otherwise), and the same tag (the ring's frame went through JPEG)
        assert [d.id() for d in det.detect_batch(imgs[:1])[0]] == [k[0] for k in want[1][1][0]]
        ring.close()
        det.close()


def test_the_file_passes_with_poisoned_allocations(built):
    """CK_POISON=1 fills every device allocation with 0xA5: nothing a call reads may be left over from before a growth."""
    if os.environ.get("CK_POISON"):
        pytest.skip("already the poisoned run")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "not poisoned"],
                       env=dict(os.environ, CK_POISON="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
