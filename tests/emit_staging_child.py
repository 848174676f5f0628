"""Child of tests/test_gpu_emit_staging.py: every frame of tests/emit_row_cases.py at the sizes of tests/emit_staging_cases.py through
AprilTagDetector.clusters on whatever build of the library the environment names (the diagnostics build with CK_EMIT_STAGE4=0,
CK_EMIT_TWINS=0 and / or CK_POISON=1), checked point for point against the oracle.
Prints one line: EMIT_STAGING_CHILD <frames checked> <points returned>."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
import emit_row_cases as ec
import emit_staging_cases as sc
from emit_rows_child import check_batch


def run():
    import pyoracle
    frames = points = 0
    for w, h in sc.SIZES:
        named = ec.frames(w, h)
        for mcp in sc.MIN_COMPONENT:
            points += check_batch(pyoracle, w, h, mcp, named)
            frames += len(named)
    print("EMIT_STAGING_CHILD", frames, points)


if __name__ == "__main__":
    run()
