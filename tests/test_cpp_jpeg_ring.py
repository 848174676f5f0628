"""The MJPEG entry points of the C++ host layer (include/chalkydri.hpp: Handle::upload_jpeg with an orientation, decode_jpeg,
IngestRing::Jpeg / write_jpeg / jpeg_status, AprilTags::process_jpeg) through tests/cpp/jpeg_ring_demo.cpp: the staged luma
byte-equal to the numpy restatement, the ring's detections byte-equal to the Python path's."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_jpeg as J  # noqa: E402
import raw_format_ref as R  # noqa: E402

from chalkydri_amd import _abi as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "chalkydri_amd", "lib", "jpeg_ring_demo")


def test_jpeg_ring_demo_refuses_a_bad_orientation(built):
    assert os.path.exists(DEMO)
    r = subprocess.run([DEMO, "upside-down", "64", "48", "1", os.devnull, os.devnull, os.devnull], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and r.stdout.startswith("PANIC"), r.stdout + r.stderr     # a Panic, as every refused call of the layer


@pytest.mark.gpu
def test_cpp_ring_equals_the_python_path(built, tmp_path):
    import scenes
    from chalkydri_amd.detector import AprilTagDetector, IngestRing
    W, H, n = 480, 360, 3
    layout = scenes.wall_layout(6, cols=3)
    r2c = {"roll": 0.0, "pitch": 0.0, "yaw": 0.0, "x": 0.2, "y": 0.0, "z": 0.6}
    frames = [scenes.render_view(300 + i, W, H, W * 0.95, layout, (2.0, 0.05 * i, 0.0), r2c, noise_amp=2)[0] for i in range(n - 1)]
    for o in R.ORIENTATIONS:
        streams = [J.encode(R.source_of(f, o), sampling=s, quality=90, restart_interval=ri) for f, s, ri in zip(frames, ("420", "grey"), (0, 4))]
        streams.append(streams[0][:len(streams[0]) // 2])          # a truncated frame: CK_JPEG_CORRUPT, zeros, no detections
        want = np.stack([R.orient_vec(J.decode_luma(b)[0], o) for b in streams[:-1]] + [np.zeros((H, W), np.uint8)])
        fin, fluma, fdets = tmp_path / "in.bin", tmp_path / "out.luma", tmp_path / "out.dets"
        fin.write_bytes(b"".join(struct.pack("<q", len(b)) + b for b in streams))
        r = subprocess.run([DEMO, o, str(W), str(H), str(n), str(fin), str(fluma), str(fdets)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
        assert np.array_equal(np.fromfile(fluma, np.uint8).reshape(n, H, W), want), o
        # the same frames through the Python ring
        det = AprilTagDetector(W, H, max_batch=n)
        ring = IngestRing(det, 1, fourcc="MJPG", orientation=o)
        for i, b in enumerate(streams):
            ring.write(0, i, b)
        ring.submit(0, n)
        cap = 64
        dets = (A.Detection * (cap * n))()
        counts = (C.c_int32 * n)()
        status = (C.c_uint32 * n)()
        assert det._L.ck_detect_ingested(ring._g, 0, n, dets, cap, counts, status) == A.CK_OK
        jst = ring.jpeg_status(0, n)
        ring.close()
        det.close()
        raw = fdets.read_bytes()
        assert raw[:4 * n] == bytes(counts)
        cpp = raw[4 * n:]
        size = C.sizeof(A.Detection)
        assert len(cpp) == size * cap * n
        for i in range(n):
            a = cpp[size * cap * i:size * (cap * i + counts[i])]
            assert a == bytes(dets)[size * cap * i:size * (cap * i + counts[i])], (o, i)
        words = r.stdout.split()[1:]
        assert words == ["%d/%d/1/1" % (jst[i], counts[i]) for i in range(n)], (o, r.stdout)
        assert jst == [0, 0, A.CK_JPEG_CORRUPT] and counts[0] > 0 and counts[1] > 0 and counts[2] == 0
