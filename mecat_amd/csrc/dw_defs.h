// dw_defs.h — what the files of the dw extension share (dw_extend.hip, dw_extend2.hip, align.hip): the workgroup shape, the block size
// of the reference, the per-direction result, the record of a handed-over unit, and the launchers' prototypes.
#pragma once
#include "common.h"

#define AL_BLOCK 256
#define AL_WAVES (AL_BLOCK / WAVE)
#define SEG_BLK 500            // DiffAlignParameters::segment_size, diff_gapalign.h:35

struct DirResult {
    int32_t qbases, tbases, matches, columns, blocks, pad;
};

// a unit dw_extend2 could not finish (a block whose tail traceback needs a row that left the ring, or that never reached an end
// of either sequence): where it stands, for dw_extend to take over
struct DwHandover {
    uint32_t unit;
    int32_t qidx, tidx;
    DirResult R;
};

// dw_extend2.hip: both directions of jobs [0, n) into dres[2 * n].  Units are pulled from *cursor; a unit the kernel cannot finish
// goes to hand[] and is counted in *hand_count (both words zeroed by the caller).
int dw_extend2_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, DirResult* dres,
                      DwHandover* hand, unsigned int* hand_count, unsigned int* cursor);
// dw_extend.hip: the same with one unit per wave and every row kept.  hand == NULL: every unit of jobs [0, n); otherwise the *hand_count
// units of hand[], from where they stand (the number is read on the device).
int dw_extend_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, DirResult* dres,
                     const DwHandover* hand, const unsigned int* hand_count, unsigned int* cursor);
