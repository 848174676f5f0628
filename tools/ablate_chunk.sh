#!/bin/bash
# cumulative cost of k_chunk's steps (quads stage time with every span cut short after step k: 1 running sums, 2 block sums,
# 3 window errors, 4 smoothing, 5 the whole kernel with k_tail ending every cluster at once as it does for 1-4, 99 everything; each
# figure from a run of its own)
# (the knob this script sets exists only in the diagnostics build of the library: ck_knobs.h)
export CHALKYDRI_HIP_LIB=${CHALKYDRI_HIP_LIB:-$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)/chalkydri_amd/lib/diag/libchalkydri_hip.so}
for k in 1 2 3 4 5 99; do
  CK_CHUNK_STOP_AFTER=$k timeout -k 10 120 python tools/bench_detect.py 1280 800 256 3 1 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('stop_after', $k, 'quads ms', d['quads'])" || exit 1
done
