"""The JPEG edge cases on the CPU (tests/jpeg_edge_cases.py): every case meets its conditions, np_jpeg's decode of it equals
libjpeg's where libjpeg takes the stream, the model's block ends equal np_jpeg's (the one place tests/jpeg_sync_model.py is itself
checked), np_jpeg.encode's new options leave its old output as it was, and the case list as a whole reaches both synchronisation
paths, every number of changing rounds, stale and empty pieces and the cap."""
import hashlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_edge_cases as EC  # noqa: E402
import jpeg_sync_model as M  # noqa: E402
import np_jpeg as J  # noqa: E402


@pytest.mark.parametrize("fam", EC.FAMILIES)
def test_cases_meet_their_conditions(fam):
    names = EC.names(fam)
    assert 0 < len(names) <= 40
    w, h = EC.SIZES[fam]
    assert w <= 264 and h <= 264
    for name in names:
        m = EC.measure(name)     # (asserts the conditions, naming the figure)
        assert m["luma"].shape == (h, w) and (m["status"] == J.OK or not m["luma"].any()), name


@pytest.mark.parametrize("fam", EC.FAMILIES)
def test_model_block_ends_equal_np_jpeg(fam):
    """The bit after the last needed block of every interval, from the model's exact chain and from np_jpeg's sequential decode;
    for a frame np_jpeg gives up on, of the intervals before the one it failed in."""
    for name in EC.names(fam):
        m = EC.measure(name)
        fig = m["fig"]
        if "refused" in fig:
            assert m["status"] != J.OK and not m["end_bits"], name
            continue
        n = len(m["end_bits"])
        assert fig["end_bits"][:n] == m["end_bits"], name
        if m["status"] == J.OK:
            assert n == fig["intervals"] and fig["blocks"] == fig["need"] and fig["short_intervals"] == 0, name
        else:
            assert n < fig["intervals"], name


@pytest.mark.parametrize("fam", EC.FAMILIES)
def test_np_jpeg_equals_libjpeg(fam):
    Image = pytest.importorskip("PIL.Image")
    compared = 0
    for name in EC.names(fam):
        m = EC.measure(name)
        if not m["libjpeg"]:
            continue
        im = Image.open(io.BytesIO(m["data"]))
        im.draft("L", im.size)
        assert np.array_equal(np.asarray(im.convert("L")), m["luma"]), name
        compared += 1
    assert compared >= len(EC.names(fam)) // 3


def test_coverage_readout():
    """Over the whole list: both paths, 0, 1, 2, 3 and >= SYNC_ROUNDS changing rounds, the walk with and without work, stale pieces,
    pieces that complete no block, blocks across two piece boundaries, intervals the cap cut."""
    figs = [EC.measure(n)["fig"] for fam in EC.FAMILIES for n in EC.names(fam)]
    figs = [f for f in figs if "refused" not in f]
    ok = [f for f in figs if f["status"] == J.OK]
    count = lambda test: sum(1 for f in ok if test(f))  # noqa: E731
    readout = {"settled": count(lambda f: f["path"] == "settled"), "walk": count(lambda f: f["path"] == "walk"),
               "walk_idle": count(lambda f: f["path"] == "walk" and f["walk_redecoded"] == 0),
               "walk_busy": count(lambda f: f["walk_redecoded"] > 0), "stale": count(lambda f: f["walk_stale"] > 0),
               "zero_block_pieces": count(lambda f: f["zero_block_pieces"] > 0), "spanning_blocks": count(lambda f: f["spanning_blocks"] > 0),
               "cap_cut": count(lambda f: f["cap_cut"] > 0), "rounds_ge_sync": count(lambda f: f["frame_rounds"] >= EC.ROUNDS),
               "rounds_eq_sync": count(lambda f: f["frame_rounds"] == EC.ROUNDS),
               "more_pieces_than_threads": count(lambda f: f["pieces"] > EC.NT), "more_intervals_than_threads": count(lambda f: f["intervals"] > EC.NT)}
    for r in range(min(EC.ROUNDS, 4)):
        readout["rounds_%d" % r] = count(lambda f: f["frame_rounds"] == r)
    print(readout)
    assert all(v > 0 for v in readout.values()), readout
    assert any(f["status"] == J.CORRUPT and f["short_intervals"] > 0 for f in figs)


def test_constants_are_the_sources():
    K = M.constants()
    assert set(K) == {"SUB_BITS", "FRAME_THREADS", "SYNC_ROUNDS", "MAX_BLOCK_BYTES"} and all(v > 0 for v in K.values())
    assert K["SUB_BITS"] % 8 == 0 and K["FRAME_THREADS"] % 64 == 0


# sha256 of np_jpeg.encode's output as it was before the append / fill / eob options existed (arguments below)
OLD_OUTPUT = {
    "420": "31471c62670dd66e42e3f31bb7abf9dba9cc0ee783504a24a5521e4a4d6b1aa0", "grey_dri": "b356a72b2fb6bd58d75fe67ff3e89c3a0779c32a6dc9576be374208db3e26279", "444_tables": "321c35faf8c0df763bd57f6da5329bb1a8175ea188106bde61ff57b6372f2239", "422_rows_q16_nodht": "40556a69472240cf05e494e80f79e6a393998ca78c6003b32ff213d166e29506", "440_dc": "f69e2f3942e9d3614a829bab4a47515e60498d100665615a26d0a427a3412d25",
}


def _old_streams():
    rng = np.random.default_rng(2024)
    img = (rng.random((40, 56)) * 256).astype(np.uint8)
    trng = np.random.default_rng(7)
    return {"420": J.encode(img), "grey_dri": J.encode(img, sampling="grey", quality=100, restart_interval=3),
            "444_tables": J.encode(img, sampling="444", quality=60, tables={(1, 0): J.shuffled_table(1, 0, trng)}),
            "422_rows_q16_nodht": J.encode(img, sampling="422", restart_interval=1, restart_rows=True, q16=True, dht=False),
            "440_dc": J.encode(img, sampling="440", quality=5, dc_offset=[-40, 0, 40])}


def test_encode_defaults_are_byte_identical():
    for name, b in _old_streams().items():
        assert hashlib.sha256(b).hexdigest() == OLD_OUTPUT[name], name
    img = np.arange(48 * 32, dtype=np.uint32).reshape(32, 48).astype(np.uint8)
    plain = J.encode(img, sampling="grey", restart_interval=4)
    assert J.encode(img, sampling="grey", restart_interval=4, append={}, fill={}, eob=0x00) == plain
    assert J.encode(img, sampling="grey", restart_interval=4, eob=0x10) == plain    # (the standard table holds no EOB-run symbol)
    more = J.encode(img, sampling="grey", restart_interval=4, append={1: b"\x01\x02", -1: b"\x03"}, fill={1: 2})
    at = EC.marker_offsets(plain)
    off = J.parse(plain)["scan_off"]
    assert more == plain[:off + at[1]] + b"\x01\x02\xff\xff" + plain[off + at[1]:-2] + b"\x03\xff\xd9"
    assert np.array_equal(J.decode_luma(more)[0], J.decode_luma(plain)[0])
