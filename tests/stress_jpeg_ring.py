"""Randomised parity stress of the oriented JPEG decode and the JPEG ingest ring: random oriented sizes 16..700, orientations,
samplings, qualities, restart intervals, table sets (standard / shuffled / absent) and slot counts.  Per case one detector and one
ring; every slot gets 1..3 streams (rendered tag scenes where the frame is large enough, texture or noise otherwise, now and then
a truncated one).  Compared, all by equality: decode_jpeg(orientation) and its status against the numpy restatement of libjpeg
(tests/np_jpeg.py) turned by tests/raw_format_ref.py; the ring's status words and detections, with every slot submitted before
the first is processed and the slots processed in reverse, against upload_jpeg + detect on the same handle.  Prints one JSON
line with the mismatch count.  usage: python tests/stress_jpeg_ring.py [cases] [seed]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import np_jpeg as J  # noqa: E402
import raw_format_ref as R  # noqa: E402
from chalkydri_amd import synth  # noqa: E402
from chalkydri_amd.detector import AprilTagDetector, IngestRing  # noqa: E402
from stress_jpeg import content  # noqa: E402


def stream(rng, S):
    """A random encoding of the source luma S; now and then cut short (CK_JPEG_CORRUPT)."""
    samp = str(rng.choice(list(J.SAMPLINGS)))
    kind = int(rng.integers(0, 4))
    kw = dict(sampling=samp, quality=int(rng.integers(1, 101)), dht=rng.random() > 0.3, q16=rng.random() < 0.2)
    if kind == 1:
        kw["restart_interval"] = int(rng.integers(1, 10))
    elif kind == 2:
        kw.update(restart_interval=int(rng.integers(1, 3)), restart_rows=True)
    if kw["dht"] and rng.random() < 0.3:
        kw["tables"] = {(c, s): J.shuffled_table(c, s, rng) for c in (0, 1) for s in (0, 1)}
    b = J.encode(S, **kw)
    if rng.random() < 0.08:
        b = b[:max(len(b) * 2 // 3, J.parse(b)["scan_off"] + 2)]
    return b


def det_key(dets):
    return [[(d.id(), d.hamming(), d.decision_margin(), d.corners().tobytes(), d.center().tobytes()) for d in f] for f in dets]


def run(cases, seed):
    rng = np.random.default_rng(seed)
    bad = frames = found = 0
    for c in range(cases):
        W, H = int(rng.integers(16, 701)), int(rng.integers(16, 701))
        o = R.ORIENTATIONS[int(rng.integers(0, 4))]
        n_slots, nb = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        slots = []
        for s in range(n_slots):
            batch = []
            for i in range(int(rng.integers(1, nb + 1))):
                if min(W, H) >= 200 and rng.random() < 0.6:
                    F = synth.render(int(rng.integers(1, 1 << 30)), W, H, int(rng.integers(1, 4)))[0][:, :W]
                else:
                    F = content(rng, H, W)
                batch.append(stream(rng, R.source_of(np.ascontiguousarray(F), o)))
            slots.append(batch)
        det = AprilTagDetector(W, H, max_batch=nb)
        ring = IngestRing(det, n_slots, fourcc="MJPG", orientation=o, max_frame_bytes=max(len(b) for batch in slots for b in batch))
        for s, batch in enumerate(slots):
            for i, b in enumerate(batch):
                ring.write(s, i, b)
            ring.submit(s, len(batch))
        got_ring = {}
        for s in reversed(range(n_slots)):
            dets, _ = ring.detect(s, len(slots[s]))
            got_ring[s] = (det_key(dets), ring.jpeg_status(s, len(slots[s])))
        for s, batch in enumerate(slots):
            luma, st = det.decode_jpeg(batch, return_status=True, orientation=o)
            n, st2 = det.upload_jpeg(batch, o, return_status=True)
            want_dets = det_key(det.detect_batch(None, n=n))
            found += sum(len(f) for f in want_dets)
            ok = got_ring[s] == (want_dets, st) and st2 == st
            for i, b in enumerate(batch):
                frames += 1
                S, wst = J.decode_luma(b)
                want = R.orient_vec(S, o) if wst == J.OK else np.zeros((H, W), np.uint8)
                ok = ok and st[i] == wst and np.array_equal(luma[i], want)
            if not ok:
                bad += 1
                print("MISMATCH case", c, "slot", s, (W, H), o, "status", st, got_ring[s][1], flush=True)
        ring.close()
        det.close()
    print(json.dumps({"stress": "jpeg_ring", "cases": cases, "seed": seed, "frames": frames, "detections": found, "mismatching": bad}), flush=True)
    return bad


if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    sys.exit(1 if run(cases, seed) else 0)
