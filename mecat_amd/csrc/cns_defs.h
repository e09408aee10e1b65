// cns_defs.h — what the files of the mecat2cns / mecat2asmpw extension share (cns_extend.hip, cns_trace.hip, cns_align.hip,
// asm_extend.hip): the block rules' two sizes, the error word of a call, and cns_extend's launcher.
#pragma once
#include "cns_fwd.h"

#define CN_SEG 500
#define CN_MAX_D 480               // int(2 * 0.20 * 1200)

// cns_trace.hip: the columns of the n_blocks block records of a forward pass (fwd: what cns_forward_launch was given), into ops
int cns_trace_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const mhip_aln_job* d_jobs, const CnsFwdArgs& fwd,
                     unsigned int n_blocks, uint32_t* ops, int* d_err);

// cns_extend.hip.  The 64-byte scratch block "cn_cursor" holds cns_extend's unit cursor in word [0] and the call's error word in word [8]
// (1: a direction needed more than dir_cols_cap columns; 3, 4: cns_trace's internal errors).
// cns_error_word says where the word is: a call zeroes it first, hands it to its kernels, and reads it behind the last one.
int cns_error_word(mhip_ctx* c, int** d_err);

// What cns_extend runs: mecat2cns' rules over mhip_aln_job (asm_rules = false) or mecat2asmpw's over mhip_asm_job (true, with the planes
// of the bases that are not A, C, G, T; launch name "asm_extend").  ulist == NULL: both directions of jobs [0, n); otherwise the units it
// lists ([0] = how many, read on the device).  Columns go to ops (dir_cols_cap / 16 words per unit, zeroed by the caller), totals to dres.
struct CnsExtendJobs {
    bool asm_rules;
    const void* d_jobs;
    int n;
    double error_rate, band_frac;
    const unsigned int* ulist;
};
// the launcher owns the grid (24 waves per CU), the per-wave rows ("cn_rows") and the cursor, which it resets
int cns_extend_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const CnsExtendJobs& jobs, int dir_cols_cap, uint32_t* ops,
                      CnsDir* dres);
