// ref_extend.h — ref_extend.hip's stage for the other stages of mecat2ref (ref_rescue.hip extends its rescue candidates with it).
#pragma once

#include "common.h"

struct RxJob {
    int64_t ref_start;           // loc1 - 1
    int32_t rid, chain, read_start, read_len;
    int32_t left, right;         // left_ref_size, right_ref_size
    int32_t valid, score;
};
struct RxDir { int32_t cols, qbases, tbases, blocks; };   // one direction as the stitching takes it

// The extension of DEVICE lists d_cands [n][maxc] / d_counts [n] (see mhip_ref_extend_run in mecat_hip.h).  `set` (0 or 1) names the
// buffers the results stay in: "rx_res", "rx_woffs" and "rx_dense" of scratch_set() and the context's rx_* members; a run into one set
// leaves the other's results fetchable.  Set 0 is mhip_ref_extend_run's, set 1 the rescue's.
// `aligner`: RX_ALIGNER_DIFF = DiffAligner (ref_extend, PacBio mode), RX_ALIGNER_XDROP = XdropAligner (ref_xextend.hip, nanopore mode);
// jobs, bounds, slices, buffer sets and the fetch are the same for both.
#define RX_ALIGNER_DIFF 0
#define RX_ALIGNER_XDROP 1
int ref_extend_run(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc, int aligner,
                   const mhip_ref_candidate* d_cands, const int32_t* d_counts, int64_t* total_words, int set);
// what mhip_ref_extend_fetch copies, of set `set`
int ref_extend_fetch(mhip_ctx* c, int set, mhip_ref_result* res, uint64_t* word_offs, uint32_t* ops_dense);

// ref_xextend.hip: units [u0, u1) of `d_jobs` through the X-drop extension on the context's stream, columns into d_store as ref_extend
// writes them (unit u from word d_dbase[u] - d_dbase[u0], the store zero-filled), directions into d_dres; *d_redone += the blocks
// redone with the wide block.  d_cursor[0] must be 0.
int ref_xextend_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const RxJob* d_jobs, unsigned int u0, unsigned int u1,
                       const unsigned long long* d_dbase, uint32_t* d_store, RxDir* d_dres, unsigned int* d_cursor, unsigned int* d_redone);
