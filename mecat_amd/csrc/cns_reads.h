// cns_reads.h — the corrected reads behind the POA (cns_reads.hip): what the host and the device share.
//
// The record rule is output_cns_result (mecat2cns/mecat_correction.cpp:155-188) as arithmetic: a segment's target of `size` letters gives
// one record when size <= 60 000; a longer one is cut into blocks of 49 000 letters that overlap by 10 000 — block k starts at L = 39 000 k
// and ends at R = L + 49 000, except that the first block with R >= size - 11 000 ends at `size` and is the last.  The reference's
// constants (MaxSeqSize, OvlpSize, BlkSize = MaxSeqSize - OvlpSize - 1000) are spelled out below.  The same two functions run in the
// record kernel and, compiled by plain g++, in libcns_poa_host.so (cns_reads_host_*), which tests/test_cns_reads_ref_cpu.py holds to the
// compiled reference's records.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CNS_READS_HD __host__ __device__
#else
#define CNS_READS_HD
#endif

enum { CNS_READS_MAX_SEQ = 60000, CNS_READS_OVLP = 10000, CNS_READS_BLK = CNS_READS_MAX_SEQ - CNS_READS_OVLP - 1000 };

// records of a target of `size` letters (size >= 1): the number of passes of the reference's do-while
CNS_READS_HD inline long long cns_reads_blocks(long long size) {
    if (size <= CNS_READS_MAX_SEQ) return 1;
    // the last block is the first k with (BLK - OVLP) k + BLK >= size - OVLP - 1000
    const long long step = CNS_READS_BLK - CNS_READS_OVLP, need = size - CNS_READS_OVLP - 1000 - CNS_READS_BLK;
    return 1 + (need + step - 1) / step;
}

// block k (0 <= k < cns_reads_blocks(size)) of a segment [beg, end): letters [*L, *R) of the target, and the record's range (:181-182)
CNS_READS_HD inline void cns_reads_block(long long size, long long k, long long beg, long long end, long long* L, long long* R, long long* range_beg, long long* range_end) {
    if (size <= CNS_READS_MAX_SEQ) { *L = 0; *R = size; *range_beg = beg; *range_end = end; return; }
    const long long l = (long long)(CNS_READS_BLK - CNS_READS_OVLP) * k;
    long long r = l + CNS_READS_BLK;
    if (r >= size - CNS_READS_OVLP - 1000) r = size;
    *L = l; *R = r;
    *range_beg = l + beg;
    *range_end = (r < size && r + beg < end) ? r + beg : end;
}

#if defined(__HIPCC__)
#include "common.h"

// One launch's reads on the device.  d_reads are final except seq_begin, which counts from the launch's first letter.
struct CnsReadsDev {
    const mhip_cns_read* d_reads = nullptr;      // [nreads] in segment order, then block order
    const char* d_seq = nullptr;                 // [seq_bytes] every kept segment's target once, in segment order
    const long long* d_tbegin = nullptr;         // [nt + 1] first record of every template of the launch, counted from the launch's first
    const long long* d_bad = nullptr;            // nonzero once the kernels have run: an index from the data left its array, or the letters
                                                 // written are not the letters counted (NULL: nothing ran)
    long long nreads = 0, seq_bytes = 0;
    double wait_s = 0;                           // host seconds spent in the wait for the two totals
};

// The corrected reads of `nseg` segments d_seg[] (a launch's part of a plan: global template numbers from t_index0, global window numbers
// from win_base, global segment numbers from seg_base; d_segb[nt + 1] the templates' first segments as global numbers) from the tables
// d_table / d_ident (template k: words [tb[k], tb[k + 1]), tb[] a HOST array relative to d_table), the windows d_win[nwin] and their
// consensus strings d_cns (window w: bytes [d_cb[w], d_cb[w + 1]), at most cns_cap in all; d_cb may be NULL when nwin == 0).  read_id[nt]
// (HOST) is what the records carry as read_id.  Everything runs on c->stream behind what the stream holds; the function WAITS for the
// stream once (the two totals size the output) and returns with the last kernel launched.  `set` (0 / 1) picks the scratch buffers.
int cns_reads_launch(mhip_ctx* c, int set, const uint32_t* d_table, const uint8_t* d_ident, int nt, int t_index0, const long long* tb, const int32_t* read_id,
                     const mhip_cns_segment* d_seg, long long nseg, const long long* d_segb, long long seg_base, long long win_base, const mhip_cns_window* d_win, long long nwin,
                     const char* d_cns, const long long* d_cb, long long cns_cap, int min_size, CnsReadsDev* out);
#endif
