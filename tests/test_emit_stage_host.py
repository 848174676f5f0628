"""Who stages what in k_emit2's group staging, without a device: the exhaustive check of ck_emit_stage.h against the per-pixel staging
the kernel keeps for widths that are no multiple of four (tests/cpp/emit_stage_check.cpp, built with AddressSanitizer + UBSan by
the Makefile).  Widths 16, 20, ... 272 by heights 16..70, every emit tile, every thread, both rounds: every cell of the 17 x 66
region written once and from the right frame pixel, every load aligned and inside its frame, the LDS words distinct, aligned and
where the count pass reads them, the per-group tile terms equal to ck_label_slot / ck_label_interior_root at each pixel."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "chalkydri_amd", "lib", "emit_stage_check")


def test_every_thread_of_every_tile_of_every_size(built):
    assert os.path.exists(CHECK)
    sym = subprocess.run(["nm", CHECK], capture_output=True, text=True).stdout
    assert "__asan_init" in sym and "__ubsan_handle" in sym          # the build that ran is the sanitized one
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout[-1500:], r.stderr[-2000:])
    print(r.stdout.strip())
