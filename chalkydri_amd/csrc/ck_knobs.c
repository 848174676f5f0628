// ck_knobs.c — ck_knob() over the table of ck_knobs.h.  Compiled twice: for the product, where a knob IS its default, and with
// -DCK_DIAG for the diagnostics library, where the environment can set it.
#include "ck_knobs.h"

#ifdef CK_DIAG
#include <stdlib.h>

enum { CK_KNOB_ONCE, CK_KNOB_PER_CALL };
#define CK_KNOB_ROW_(id, dflt, read, about) {"CK_" #id, dflt, CK_KNOB_##read, about},
static const struct { const char *name; int dflt, read; const char *about; } knobs[CK_KNOB_COUNT] = {CK_KNOB_TABLE(CK_KNOB_ROW_)};

int ck_knob(int id) {
    const char *e = getenv(knobs[id].name);
    return e ? (int)strtol(e, NULL, 10) : knobs[id].dflt;
}
#else
#define CK_KNOB_ROW_(id, dflt, read, about) dflt,
static const int knobs[CK_KNOB_COUNT] = {CK_KNOB_TABLE(CK_KNOB_ROW_)};

int ck_knob(int id) { return knobs[id]; }
#endif
