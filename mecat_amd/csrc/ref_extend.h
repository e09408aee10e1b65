// ref_extend.h — ref_extend.hip's stage for the other stages of mecat2ref (ref_rescue.hip extends its rescue candidates with it).
#pragma once

#include "common.h"

// The extension of DEVICE lists d_cands [n][maxc] / d_counts [n] (see mhip_ref_extend_run in mecat_hip.h).  `set` (0 or 1) names the
// buffers the results stay in: "rx_res", "rx_woffs" and "rx_dense" of scratch_set() and the context's rx_* members; a run into one set
// leaves the other's results fetchable.  Set 0 is mhip_ref_extend_run's, set 1 the rescue's.
int ref_extend_run(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc, int tech,
                   const mhip_ref_candidate* d_cands, const int32_t* d_counts, int64_t* total_words, int set);
// what mhip_ref_extend_fetch copies, of set `set`
int ref_extend_fetch(mhip_ctx* c, int set, mhip_ref_result* res, uint64_t* word_offs, uint32_t* ops_dense);
