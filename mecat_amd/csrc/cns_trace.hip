// cns_trace.hip — the paths of the mecat2cns re-aligner (cns_fwd.h): from the row log and block records the forward pass
// (cns_forward, dw_extend2.hip) left, to the 2-bit columns of every block.
#include "cns_defs.h"
#include "dw_helpers.h"

// cns_trace — one LANE per block record.  Backwards over the block's row records from its end cell: bit (k - min_k) / 2 of a row says
// which neighbour of the row below the cell came from (the reference's traceback reads the same off its stored V values, dw.cpp:222-240),
// min_k of the row below follows from that row's cut; the steps go into a per-lane bit array in LDS.  Forwards again from (0, 0): row d
// is one column with a base of one sequence only — the query's when the step came from k - 1 — and then the snake, re-measured on the
// packed reads (the forward pass compared exactly these bases); columns at or beyond kept_cols (the cut in front of the last four
// matches) are dropped.  Columns: 0 = both bases (the buffer is zero-filled), 1 = target base only, 2 = query base only.
#define CT_BLOCK 256
#define CT_WORDS ((CN_MAX_D + 31) / 32)
__global__ __launch_bounds__(CT_BLOCK) void cns_trace(const uint32_t* __restrict__ rpac, const mhip_offset_t* __restrict__ roffs,
                                                      const uint32_t* __restrict__ qpac, const mhip_offset_t* __restrict__ qoffs,
                                                      const mhip_aln_job* __restrict__ jobs, const CnsBlockRec* __restrict__ blocks, unsigned int nb,
                                                      const CnsRowRec* __restrict__ rowlog, CnsDir* __restrict__ dres, uint32_t* __restrict__ ops,
                                                      size_t dir_words, int* __restrict__ err_flag) {
    __shared__ uint32_t path[CT_BLOCK / 64][CT_WORDS][64];
    const int lane = lane_id(), wv = (int)threadIdx.x >> 6;
    for (unsigned int b0 = blockIdx.x * CT_BLOCK; b0 < nb; b0 += gridDim.x * CT_BLOCK) {
        const unsigned int b = b0 + threadIdx.x;
        if (b >= nb) continue;
        const CnsBlockRec B = blocks[b];
        if (B.unit == 0xffffffffu) continue;                     // (a record of its unit's share that no block took)
        if (dres[B.unit].pad < 0 || B.end_d >= CN_MAX_D) {      // (a unit that was handed over after this block: cns_extend redoes it)
            if (B.end_d >= CN_MAX_D) atomicExch(err_flag, 3);
            continue;
        }
        // ---- backwards: the steps
        // The records of rows end_d .. 1 are read in aligned groups of four (64 bytes, four 16-byte loads of one line): a lane that fetched
        // one record per step pulled the same line in from memory up to four times (the lanes of a wave walk 64 different blocks; r05:
        // 62.9 GB fetched for 19 GB of records).  Row d's first diagonal follows from row d + 1's by row d's own cut, so a record is all
        // a step needs.
        {
            int ck = B.end_k, mk = B.end_mk, wi = B.end_d >> 5;
            uint32_t word = 0;
            bool bad = false;
            unsigned int rec = B.log0 + (unsigned)B.end_d;                 // record of the row in hand
            const unsigned int rec_last = B.log0 + 1u;                     // record of row 1
            const uint4* log4 = (const uint4*)rowlog;
            while (rec >= rec_last && B.end_d >= 1) {
                const unsigned int g = rec & ~3u;
                uint4 R4[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) R4[k] = log4[g + (unsigned)k];      // (records in front of the block or behind its end row: loaded, not used)
#pragma unroll
                for (int k = 3; k >= 0; --k) {
                    const unsigned int r = g + (unsigned)k;
                    if (r > rec || r < rec_last) continue;
                    const uint4 R = R4[k];                                   // {lo, hi, meta, top}
                    const int cd = (int)(r - B.log0);
                    if (cd != B.end_d) mk = mk - 2 * (int)((R.z >> 8) & 0x7fu) + 1;
                    const int t = (ck - mk) >> 1;
                    bad |= t < 0 || t >= (int)(R.z & 0xffu);                 // (never: the path stays inside its rows)
                    const uint32_t bit = ((t < 32 ? R.x : t < 64 ? R.y : R.w) >> (t & 31)) & 1u;
                    if ((cd >> 5) != wi) { path[wv][wi][lane] = word; word = 0; wi = cd >> 5; }
                    word |= bit << (cd & 31);
                    ck += bit ? -1 : 1;
                }
                if (g <= rec_last) break;
                rec = g - 1u;
            }
            path[wv][wi][lane] = word;
            if (bad) atomicExch(err_flag, 3);
        }
        // ---- forwards: the columns
        const mhip_aln_job jb = jobs[B.unit >> 1];
        const int right = (int)(B.unit & 1u);
        SeqView q, t;
        q.pac = qpac; t.pac = rpac;
        {
            const int qsize = qoffs[jb.qid_local].size;
            q.off = qoffs[jb.qid_local].offset; q.comp = jb.chain;
            t.off = roffs[jb.sid_local].offset; t.comp = 0;
            const int qs0 = right ? jb.qstart : jb.qstart - 1, step = right ? 1 : -1;
            if (jb.chain) { q.A = qsize - 1 - qs0; q.B = -step; } else { q.A = qs0; q.B = step; }
            t.A = right ? jb.sstart : jb.sstart - 1; t.B = step;
        }
        uint32_t* uops = ops + (size_t)B.unit * dir_words;
        int x = 0, y = 0, c = 0, n_ins = 0, n_del = 0;
        // 32 bases of either sequence stay in two registers (bases qb .. qb + 31 of the block, first base in the low bits): a row moves
        // along by three or four bases, so a window is refilled once in four rows instead of being fetched and turned for every snake step
        int qb = 0, tb = 0;
        uint32_t q0 = view_word_le(q, B.qidx), q1 = view_word_le(q, B.qidx + 16), t0 = view_word_le(t, B.tidx), t1 = view_word_le(t, B.tidx + 16);
        auto snake = [&]() {
            const int lim = min(B.seg - x, B.seg - y);
            int run = 0;
            while (run < lim) {
                const int xx = x + run, yy = y + run;
                while (xx >= qb + 16) { qb += 16; q0 = q1; q1 = view_word_le(q, B.qidx + qb + 16); }
                while (yy >= tb + 16) { tb += 16; t0 = t1; t1 = view_word_le(t, B.tidx + tb + 16); }
                const uint32_t dlt = __builtin_amdgcn_alignbit(q1, q0, (uint32_t)(xx - qb) << 1) ^ __builtin_amdgcn_alignbit(t1, t0, (uint32_t)(yy - tb) << 1);
                const int m = min(dlt ? (__builtin_ctz(dlt) >> 1) : 16, lim - run);
                run += m;
                if (m < 16) break;
            }
            x += run; y += run; c += run;
        };
        // the columns of a word are gathered in a register and written once: with a plain store when the word is this block's alone, with
        // an atomic OR when it holds the block's first or last kept column (its neighbours in the unit write the rest of it)
        const int gc_lo = B.col0, gc_hi = B.col0 + B.kept_cols - 1;
        int cw = gc_lo >> 4;
        uint32_t wacc = 0;
        auto flush_word = [&]() {
            if (wacc) {
                if (cw == (gc_lo >> 4) || cw == (gc_hi >> 4)) atomicOr(&uops[cw], wacc); else uops[cw] = wacc;
            }
            wacc = 0;
        };
        snake();
        for (int d = 1; d <= B.end_d && c < B.kept_cols; ++d) {
            const uint32_t bit = (path[wv][d >> 5][lane] >> (d & 31)) & 1u;
            x += (int)bit; y += 1 - (int)bit;
            n_del += (int)bit; n_ins += 1 - (int)bit;
            const int gc = B.col0 + c;
            if ((gc >> 4) != cw) { flush_word(); cw = gc >> 4; }
            wacc |= (bit ? 2u : 1u) << ((gc & 15) << 1);
            c += 1;
            snake();
        }
        flush_word();
        if (B.kept_cols == (B.end_x + (B.end_x - B.end_k) + B.end_d) / 2 && x != B.end_x) atomicExch(err_flag, 4);      // (a whole block ends in its end cell)
        if (n_ins) atomicAdd(&dres[B.unit].ins, n_ins);
        if (n_del) atomicAdd(&dres[B.unit].del, n_del);
    }
}

int cns_trace_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const mhip_aln_job* d_jobs, const CnsFwdArgs& fwd,
                     unsigned int n_blocks, uint32_t* ops, int* d_err) {
    LAUNCH(c, "cns_trace", cns_trace, c->num_cus * 8, CT_BLOCK, 0, (const uint32_t*)ref->d_pac, (const mhip_offset_t*)ref->d_offs,
           (const uint32_t*)reads->d_pac, (const mhip_offset_t*)reads->d_offs, d_jobs, (const CnsBlockRec*)fwd.blocks, n_blocks,
           (const CnsRowRec*)fwd.rowlog, fwd.dres, ops, (size_t)fwd.dir_cols_cap / 16, d_err);
    return 0;
}
