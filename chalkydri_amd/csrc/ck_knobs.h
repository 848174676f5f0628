// ck_knobs.h — the diagnostic knobs: kernels cut short, classes skipped, paths forced, launch geometry varied.  One table, below.
//
// A knob is an environment variable of the DIAGNOSTICS library alone (`make diag` -> chalkydri_amd/lib/diag/libchalkydri_hip.so), which
// the measurement scripts under tools/ and the path-forcing tests load.  That library is the product's own object files with two
// exceptions, the two units compiled a second time with -DCK_DIAG: ck_knobs.c, whose ck_knob() reads the environment there, and
// k_chunk.hip, whose kernels are the only device code a knob changes.  In the product ck_knob() returns the default: ck_knobs.o holds
// neither the names nor a getenv call, so the environment cannot change what the drop-in returns.  The product library reads exactly
// one variable, which is no knob: CK_POISON (ck_internal.h: allocation fill / guard pages).
//
// ONCE: the one site that reads the knob keeps the value in a `static const int` — the environment at the first call counts.
// PER_CALL: read by every call, so that a test can change it between two calls of one process.
#ifndef CK_KNOBS_H
#define CK_KNOBS_H

//  id                 default  read      what it does
#define CK_KNOB_TABLE(X) \
    X(TILE_STOP_AFTER,   99, ONCE,     "k_tile ends after phase k (k_ccl.hip); 99 = all of it") \
    X(FMERGE_STOP_AFTER, 99, ONCE,     "k_fmerge ends after step k (k_ccl.hip); 99 = all of it") \
    X(FMERGE_CAP,         0, PER_CALL, "roots k_fmerge's LDS path holds, when smaller than the computed capacity: forces the global-memory path") \
    X(FMERGE_BAND_ROWS,   0, PER_CALL, "tile rows per band of the segmentation's merge; 0 = the computed height") \
    X(EMIT_STOP_AFTER,   99, ONCE,     "k_emit2 ends after phase k (k_clusters.hip); 99 = all of it") \
    X(EMIT_TWINS,         1, ONCE,     "0 = k_emit2 stores every point on its own instead of diagonal twins as one word; 2 = twins as one word, but the quad fit keeps the duplicate removal it needs for 0 (FitArgs::distinct off)") \
    X(EMIT_STAGE4,        1, ONCE,     "0 = k_emit2 stages every pixel on its own instead of aligned groups of four") \
    X(FIT_SPLIT,          3, ONCE,     "bit 0 = 513..1024 points have a size class of their own, bit 1 = up to 256 points have") \
    X(FIT_FLAT,           1, ONCE,     "the split fit (k_seq, k_chunk, k_tail): 0 never, 2 always, 1 = for the calls it pays for") \
    X(FIT_SKIP,           0, ONCE,     "bit c set = size class c of the quad fit is not launched") \
    X(CHUNK_WGS,         64, ONCE,     "k_chunk workgroups per CU over the batch") \
    X(FIT_STOP_AFTER,    99, PER_CALL, "every cluster of the quad fit ends after phase k (k_quads.hip); 99 = all of it") \
    X(EXT_BASE,           0, PER_CALL, "first position of the split fit's extended sequences in every frame, 0 .. 2 * CK_SPAN (k_chunk.hip)") \
    X(CHUNK_STOP_AFTER,  99, PER_CALL, "every span of k_chunk ends after step k (k_chunk.hip); 99 = all of it")

#define CK_KNOB_ID_(id, dflt, read, about) CK_KNOB_##id,
enum ck_knob_id { CK_KNOB_TABLE(CK_KNOB_ID_) CK_KNOB_COUNT };
#undef CK_KNOB_ID_

#ifdef __cplusplus
extern "C"
#endif
int ck_knob(int id); // the knob's value: its default; in the diagnostics build the decimal number in the variable CK_<id> where that is set

#endif
