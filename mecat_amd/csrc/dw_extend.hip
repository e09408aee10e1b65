// dw_extend.hip — "dw", the one-unit kernel: banded O(ND) furthest-reaching d-path local aligner in 500-bp blocks (SURVEY.md §8a rows
// A10-A12), one wave per (candidate, direction), every d-row kept.
//
// Today it is the second launch of the two-launch scheme (align.hip): dw_extend2 (dw_extend2.hip) runs all units, two per wave, and
// hands over the ~0.5 % it cannot finish — a tail traceback that needs a row its ring no longer holds, a block that reached no end of
// either sequence — with where they stand (DwHandover); this kernel finishes them.  MECAT_DW_KERNEL=1 runs every unit through it (the
// tests compare the two).
//
// Replaces, for PacBio-mode candidates (pairwise_mapping, mecat2pw/pw_impl.cpp:674-698):
//   DiffAligner::go          common/diff_gapalign.cpp:294-349   left + right extension from the seed point, stitching
//   dw_in_one_direction      common/diff_gapalign.cpp:221-292   block chaining with the 4-match tail anchor
//   retrieve_next_aln_block  common/gapalign.cpp:9-45           500-bp blocks, last-block sizing
//   Align                    common/diff_gapalign.cpp:107-219   O(ND) wavefront with the adaptive band
//   GetAlignString           common/diff_gapalign.cpp:39-104    traceback
//   trim_mismatch_end        common/gapalign.cpp:47-68          tail anchor
//
// mecat2pw consumes only the four end coordinates and the identity (matches / columns) of an alignment, never the
// aligned strings, so the traceback is reduced to what those need.  An O(ND) path is a chain of d+1 match runs
// ("snakes") separated by single-base indels, hence per block
//     columns = (x + y + d) / 2,  matches = (x + y - d) / 2                       (Align: aln_str_size)
// and trim_mismatch_end (4 consecutive equal columns from the tail) is "walk the path back to the first snake of
// length >= 4".  Only that tail of the path is traced.
//
// Mapping: a direction is a sequential chain of blocks; inside a block the d-loop is sequential and the <= 217 diagonals of the band
// are the lanes (up to 4 per lane).  Per-wave LDS (9.2 KB):
//   V[]      furthest x per diagonal (int16; x + y is recomputed as 2x - k, no U array)
//   Qp/Tp    the two block sequences, 2 bits per base MSB-first, staged straight from the packed volume with two
//            word loads per lane (reverse / reverse-complement views by a 2-bit-group reversal and a bit complement)
//   ring     the most recent 16 d-rows (u16 x per diagonal) + their band limits, for the tail traceback
// Snakes compare 32 bases per step: XOR of unaligned 32-bit windows + count-leading-zeros.  A path whose last >= 4 snake is more than
// 16 rows back re-runs the block with all rows spilled to a per-wave global scratch ("al_rows").  Waves are persistent and pull units
// from an atomic cursor; dw_stitch (align.hip) joins the two directions.
#include <stdlib.h>

#include <algorithm>

#include "dw_defs.h"

#define MAX_BLK 736            // last block (gapalign.cpp:24-30): one side < 600, the other <= int(599 * 1.2) = 718
#define SEQ_WORDS 52           // 736 / 16 = 46 words + window slack
#define MAX_D 400              // int(0.3 * (599 + 718)) = 395
#define VU_LEN (2 * MAX_D + 8)
#define ROW_W 224              // diagonals per d-row: (2 * int(0.3 * 718)) / 2 + 1 = 216
#define RING 16
#define GROW_STRIDE ((size_t)MAX_D * ROW_W + 2 * (MAX_D + 8))   // u16 per wave: rows + rmin + rmax

struct AlnWaveLds {
    uint32_t Qp[SEQ_WORDS];     // staged block sequences first: their byte offsets fit the ds_read2 offset field
    uint32_t Tp[SEQ_WORDS];
    int16_t V[VU_LEN];
    uint16_t ring[RING * ROW_W];
    int16_t rmin[RING];
    int16_t rmax[RING];
};

#include "dw_helpers.h"

// One d-row for NJ diagonals per lane (straight-line: lanes past the last diagonal recompute the last one -- same
// addresses, same values -- so nothing is predicated per lane).  Returns the wave-reduced keys
//   bkey = (x+y) << 10 | (1023 - (k + k_offset))   max  -> first maximum of x + y in k order (diff_gapalign.cpp:160-167)
//   hkey = (k + k_offset) << 10 | x                min  -> lowest diagonal that reached an end (:168-169), or INT_MAX
// and leaves x + y of the lane's diagonals in S-independent registers via xy[] for the band update.
template <int NJ, bool SPILL>
__device__ __forceinline__ void row_body(AlnWaveLds& S, uint16_t* __restrict__ grow, const int lane, const int d, const int nslot,
                                         const int min_k, const int max_k, const int k_offset, const int q_len, const int t_len,
                                         const int best_m, const int band_tol, unsigned int& snake, int& bkey_out, int& hkey_out,
                                         int& x0_out) {
    int xs[NJ], ys[NJ], kks[NJ];
    // start points (:138-142)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int t = min(lane + 64 * j, nslot - 1);
        const int k = min_k + 2 * t;
        kks[j] = k + k_offset;
        const int vl = S.V[k - 1 + k_offset], vr = S.V[k + 1 + k_offset];
        const int x = (k == min_k || (k != max_k && vl < vr)) ? vr : vl + 1;
        xs[j] = x; ys[j] = x - k;
    }
    // snakes, 32 bases per round; a round is idempotent for a diagonal that already stopped
    bool more;
    do {
        more = false;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int x = xs[j], y = ys[j];
            const int lim = min(q_len - x, t_len - y);
            const int n0 = match32(S.Qp, x, S.Tp, min(y, MAX_BLK));
            const int n = max(0, min(n0, lim));
            xs[j] = x + n; ys[j] = y + n;
            snake += (unsigned int)n;
            more |= (n == 32) & (lim > 32);
        }
    } while (__ballot(more));
    __builtin_amdgcn_wave_barrier();
    int bkey = -1, hkey = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int t = min(lane + 64 * j, nslot - 1);
        S.V[kks[j]] = (int16_t)xs[j];
        if (SPILL) grow[(size_t)d * ROW_W + t] = (uint16_t)xs[j];
        else S.ring[(d % RING) * ROW_W + t] = (uint16_t)xs[j];
        bkey = max(bkey, ((xs[j] + ys[j]) << 10) | (1023 - kks[j]));
        hkey = min(hkey, (xs[j] >= q_len || ys[j] >= t_len) ? ((kks[j] << 10) | xs[j]) : 0x7fffffff);
    }
    bkey_out = wave_max(bkey);
    hkey_out = wave_min(hkey);
    x0_out = xs[0];
}

// Fast d-row: at most 64 diagonals and the band's left edge moved by -1 (no pruning on the left, SHL = false) or by +1
// (one diagonal pruned on the left, SHL = true).  The previous row is still in a register: diagonal k of this row sits
// in the lane that held k+1 (SHL = false) resp. k-1 (SHL = true) in the previous row, and the other neighbour is one
// lane away: one wave_shr:1 / wave_shl:1 DPP move replaces the two LDS reads of V.  The lowest end-reaching diagonal
// and the first maximum are found with ballots (lane order == diagonal order) instead of key reductions.
template <bool SPILL, bool SHL>
__device__ __forceinline__ void row_fast(AlnWaveLds& S, uint16_t* __restrict__ grow, const int lane, const int d, const int nslot,
                                         const int min_k, const int max_k, const int k_offset, const int q_len, const int t_len,
                                         unsigned int& snake, int& xreg, int& m_out, int& bkey_out, int& hkey_out) {
    const bool act = lane < nslot;
    const int k = min_k + 2 * lane;
    int vl, vr;
    if (SHL) { vl = xreg; vr = __builtin_amdgcn_update_dpp(0, xreg, 0x130 /* wave_shl:1 */, 0xF, 0xF, false); }
    else { vr = xreg; vl = __builtin_amdgcn_update_dpp(0, xreg, 0x138 /* wave_shr:1 */, 0xF, 0xF, false); }
    int x = (lane == 0 || (k != max_k && vl < vr)) ? vr : vl + 1;       // :138-142
    x = act ? x : 0;
    int y = act ? x - k : 0;
    bool more;
    do {
        const int lim = min(q_len - x, t_len - y);
        const int n0 = match32(S.Qp, x, S.Tp, min(y, MAX_BLK));
        const int n = max(0, min(n0, lim));
        x += n; y += n;
        snake += (unsigned int)n;           // inactive lanes sit at (0, 0) of both sequences; corrected below
        more = (n == 32) & (lim > 32);
    } while (__ballot(more) & (nslot >= 64 ? ~0ull : ((1ull << nslot) - 1ull)));
    __builtin_amdgcn_wave_barrier();
    if (act) {
        S.V[k + k_offset] = (int16_t)x;
        if (SPILL) grow[(size_t)d * ROW_W + lane] = (uint16_t)x;
        else S.ring[(d % RING) * ROW_W + lane] = (uint16_t)x;
    } else snake -= (unsigned int)x;        // what the idle lane "matched" from (0, 0)
    const unsigned long long amask = nslot >= 64 ? ~0ull : ((1ull << nslot) - 1ull);
    const int m = act ? x + y : -1;
    const int rm = wave_max(m);
    const int lb = __ffsll((unsigned long long)(__ballot(m == rm) & amask)) - 1;          // first maximum in k order
    bkey_out = (rm << 10) | (1023 - (min_k + 2 * lb + k_offset));
    const unsigned long long hb = __ballot(x >= q_len || y >= t_len) & amask;              // lowest diagonal that reached an end
    if (hb) {
        const int lh = __ffsll(hb) - 1;
        hkey_out = ((min_k + 2 * lh + k_offset) << 10) | __builtin_amdgcn_readlane(x, lh);
    } else hkey_out = 0x7fffffff;
    xreg = x;
    m_out = m;
}

// band update (:172-179) on U[k] = x + y = 2 V[k] - k of the row just written.  Neutral elements are the reference's
// initial values (new_min_k = max_k, new_max_k = min_k).
template <bool SPILL>
__device__ __forceinline__ void band_keys(AlnWaveLds& S, const int lane, const int nj, const int nslot, const int min_k, const int max_k,
                                          const int k_offset, const int best_m, const int band_tol, int& nmin, int& nmax) {
    int lo = max_k, hi = min_k;
    for (int j = 0; j < nj; ++j) {
        const int t = min(lane + 64 * j, nslot - 1);
        const int k = min_k + 2 * t;
        const bool q = 2 * (int)S.V[k + k_offset] - k >= best_m - band_tol;
        lo = min(lo, q ? k : max_k);
        hi = max(hi, q ? k : min_k);
    }
    nmin = wave_min(lo);
    nmax = wave_max(hi);
}

struct DwStats { unsigned int rows, fast_rows, wide_rows, unaligned, spills; };

struct BlockOut {
    int aligned_or_best;   // 1 when an alignment exists (aln_str_size > 0 possible)
    int qe, te, dist;      // aln_q_e, aln_t_e, dist
    int qcnt, tcnt, acnt;  // trim_mismatch_end outputs
    int trim_ok;
    int fallback;          // ring too short for the tail traceback
};

// One block: Align + tail traceback + trim_mismatch_end.  SPILL = false: d-rows in the LDS ring; true: in global rows.
template <bool SPILL>
__device__ void align_block(AlnWaveLds& S, const int q_len, const int t_len, uint16_t* __restrict__ grow, BlockOut& o,
                            unsigned int& cells, unsigned int& snake, DwStats& st) {
    const int lane = lane_id();
    const int band_tol = (int)(0.3 * (q_len > t_len ? q_len : t_len));      // dw_in_one_direction passes 0.3 * max(qblk, tblk)
    const int max_d = (int)(.3 * (q_len + t_len));
    const int k_offset = max_d;
    const int band_size = band_tol * 2;
    int16_t* g_rmin = (int16_t*)(grow + (size_t)MAX_D * ROW_W);
    int16_t* g_rmax = g_rmin + (MAX_D + 8);
    for (int i = lane; i < 2 * max_d + 4 && i < VU_LEN; i += 64) S.V[i] = 0;     // V is zero-filled per block (:232-233)
    __builtin_amdgcn_wave_barrier();
    int best_m = -1, best_x = -1, best_y = -1, best_d = 0, best_k = 0;
    int min_k = 0, max_k = 0;
    int aligned = 0, end_x = 0, end_y = 0, end_d = 0, end_k = 0;
    o.fallback = 0;
    int d, last_row = -1;
    int xreg = 0, reg_min_k = 0;      // previous row's x per lane (valid when that row had <= 64 diagonals)
    bool reg_ok = false;
    for (d = 0; d < max_d; ++d) {
        if (max_k - min_k > band_size) break;
        last_row = d;
        const int nslot = (max_k - min_k) / 2 + 1;
        const int nj = (nslot + 63) >> 6;            // diagonals per lane this row (uniform)
        if (lane == 0) {
            if (SPILL) { g_rmin[d] = (int16_t)min_k; g_rmax[d] = (int16_t)max_k; }
            else { S.rmin[d % RING] = (int16_t)min_k; S.rmax[d % RING] = (int16_t)max_k; }
        }
        int bkey, hkey, x0 = 0, mreg = 0;
        const bool fast_r = nj == 1 && reg_ok && min_k == reg_min_k - 1;
        const bool fast_l = nj == 1 && reg_ok && min_k == reg_min_k + 1 && nslot <= 63;
        const bool fast = fast_r || fast_l;
        if (fast_r) {
            row_fast<SPILL, false>(S, grow, lane, d, nslot, min_k, max_k, k_offset, q_len, t_len, snake, xreg, mreg, bkey, hkey);
        } else if (fast_l) {
            row_fast<SPILL, true>(S, grow, lane, d, nslot, min_k, max_k, k_offset, q_len, t_len, snake, xreg, mreg, bkey, hkey);
        } else {
            switch (nj) {
            case 1: row_body<1, SPILL>(S, grow, lane, d, nslot, min_k, max_k, k_offset, q_len, t_len, best_m, band_tol, snake, bkey, hkey, x0); break;
            case 2: row_body<2, SPILL>(S, grow, lane, d, nslot, min_k, max_k, k_offset, q_len, t_len, best_m, band_tol, snake, bkey, hkey, x0); break;
            case 3: row_body<3, SPILL>(S, grow, lane, d, nslot, min_k, max_k, k_offset, q_len, t_len, best_m, band_tol, snake, bkey, hkey, x0); break;
            default: row_body<4, SPILL>(S, grow, lane, d, nslot, min_k, max_k, k_offset, q_len, t_len, best_m, band_tol, snake, bkey, hkey, x0); break;
            }
            xreg = x0;
        }
        bkey = __builtin_amdgcn_readfirstlane(bkey);      // wave-uniform: keep the bookkeeping on the scalar unit
        hkey = __builtin_amdgcn_readfirstlane(hkey);
        reg_ok = nj == 1;
        reg_min_k = min_k;
        st.rows += 1; st.fast_rows += fast ? 1u : 0u; st.wide_rows += nj > 1 ? 1u : 0u;
        cells += (unsigned int)nslot;
        {
            const int rm = bkey >> 10, rk = 1023 - (bkey & 1023) - k_offset;
            if (rm > best_m) { best_m = rm; best_x = (rm + rk) / 2; best_y = best_x - rk; best_d = d; best_k = rk; }
        }
        // band update (:172-179): needs the new best_m.  When both outermost diagonals qualify, so does the whole range.
        int nmin, nmax;
        bool whole = false;
        if (fast) {
            const int m0 = __builtin_amdgcn_readlane(mreg, 0), ml = __builtin_amdgcn_readlane(mreg, nslot - 1);
            whole = m0 >= best_m - band_tol && ml >= best_m - band_tol;
        }
        if (whole) { nmin = min_k; nmax = max_k; }
        else band_keys<SPILL>(S, lane, nj, nslot, min_k, max_k, k_offset, best_m, band_tol, nmin, nmax);
        max_k = __builtin_amdgcn_readfirstlane(nmax) + 1;
        min_k = __builtin_amdgcn_readfirstlane(nmin) - 1;
        __builtin_amdgcn_wave_barrier();
        if (hkey != 0x7fffffff) {
            aligned = 1; end_k = (hkey >> 10) - k_offset; end_x = hkey & 1023; end_y = end_x - end_k; end_d = d;
            break;
        }
    }
    o.trim_ok = 0; o.qcnt = o.tcnt = o.acnt = 0;
    if (!aligned) {
        st.unaligned += 1;
        if (best_x > 0) { end_x = best_x; end_y = best_y; end_d = best_d; end_k = best_k; }
        else { o.aligned_or_best = 0; o.qe = o.te = o.dist = 0; return; }
    }
    o.aligned_or_best = 1; o.qe = end_x; o.te = end_y; o.dist = end_d;
    // ---- tail traceback == trim_mismatch_end(.., 4, ..) on the alignment string (gapalign.cpp:47-68)
    const int aln_size = (end_x + end_y + end_d) / 2;
    int cd = end_d, ck = end_k, cx2 = end_x;
    int qcnt = 0, tcnt = 0, acnt = 0, found = 0;
    while (true) {
        int x1, pre_k = 0, takes_q = 0;
        if (cd == 0) x1 = 0;   // V is zero-filled: the d = 0 point starts at (0, 0)
        else {
            if (!SPILL && last_row - (cd - 1) >= RING) { o.fallback = 1; return; }
            int pmin, pmax, cmin, cmax, vl = 0, vr = 0;
            const int kl = ck - 1, kr = ck + 1;
            // values the forward pass read: row d-1 inside its band (always the case), else the zero fill
            if (SPILL) {
                pmin = g_rmin[cd - 1]; pmax = g_rmax[cd - 1]; cmin = g_rmin[cd]; cmax = g_rmax[cd];
                const uint16_t* prow = grow + (size_t)(cd - 1) * ROW_W;
                if (kl >= pmin && kl <= pmax) vl = prow[(kl - pmin) >> 1];
                if (kr >= pmin && kr <= pmax) vr = prow[(kr - pmin) >> 1];
            } else {
                pmin = S.rmin[(cd - 1) % RING]; pmax = S.rmax[(cd - 1) % RING]; cmin = S.rmin[cd % RING]; cmax = S.rmax[cd % RING];
                const uint16_t* prow = S.ring + ((cd - 1) % RING) * ROW_W;
                if (kl >= pmin && kl <= pmax) vl = prow[(kl - pmin) >> 1];
                if (kr >= pmin && kr <= pmax) vr = prow[(kr - pmin) >> 1];
            }
            if (ck == cmin || (ck != cmax && vl < vr)) { x1 = vr; pre_k = kr; takes_q = 0; }
            else { x1 = vl + 1; pre_k = kl; takes_q = 1; }
        }
        const int s = cx2 - x1;     // snake length
        if (s >= 4) { acnt += 4; qcnt += 4; tcnt += 4; found = 1; break; }
        acnt += s; qcnt += s; tcnt += s;
        if (cd == 0) break;
        acnt += 1;                  // the indel column
        if (takes_q) { qcnt += 1; cx2 = x1 - 1; } else { tcnt += 1; cx2 = x1; }
        ck = pre_k;
        --cd;
    }
    o.qcnt = qcnt; o.tcnt = tcnt; o.acnt = acnt;
    o.trim_ok = found && (aln_size - acnt >= 2);     // "m == mat_cnt && k > 0"
}

__global__ __launch_bounds__(AL_BLOCK) void dw_extend(const uint32_t* __restrict__ rpac, const mhip_offset_t* __restrict__ roffs,
                                                      const uint32_t* __restrict__ qpac, const mhip_offset_t* __restrict__ qoffs,
                                                      const mhip_aln_job* __restrict__ jobs, int n, DirResult* __restrict__ dres,
                                                      uint16_t* __restrict__ gscratch, unsigned int* __restrict__ cursor,
                                                      unsigned long long* __restrict__ counters, const DwHandover* __restrict__ hand,
                                                      const unsigned int* __restrict__ hand_count) {
    __shared__ AlnWaveLds lds[AL_WAVES];
    AlnWaveLds& S = lds[threadIdx.x >> 6];
    const int lane = lane_id();
    const int gw = blockIdx.x * AL_WAVES + (threadIdx.x >> 6);
    uint16_t* grow = gscratch + (size_t)gw * GROW_STRIDE;
    unsigned long long cells = 0, snake = 0, nblocks = 0, nfallback = 0;
    unsigned int ucells = 0, usnake = 0;
    DwStats st = {0, 0, 0, 0, 0};
    while (true) {
        unsigned int unit = 0;
        if (lane == 0) unit = atomicAdd(cursor, 1u);
        unit = __shfl(unit, 0);
        int qidx = 0, tidx = 0;
        DirResult R = {0, 0, 0, 0, 0, 0};
        if (hand) {                                   // second launch: the units dw_extend2 handed over, from where they stand
            if (unit >= *hand_count) break;
            const DwHandover h = hand[unit];
            unit = h.unit; qidx = h.qidx; tidx = h.tidx; R = h.R;
        } else if (unit >= 2u * (unsigned)n) break;
        const mhip_aln_job jb = jobs[unit >> 1];
        const int right = unit & 1;
        const int qsize = qoffs[jb.qid_local].size, tsize = roffs[jb.sid_local].size;
        // extension views: logical position i of the query is strand position qstart + i (right) or qstart - 1 - i (left);
        // strand position p of a reverse-complemented query is original index qsize - 1 - p, complemented
        SeqView q, t;
        q.pac = qpac; q.off = qoffs[jb.qid_local].offset; q.comp = jb.chain;
        t.pac = rpac; t.off = roffs[jb.sid_local].offset; t.comp = 0;
        int query_size, target_size;
        const int qs0 = right ? jb.qstart : jb.qstart - 1, step = right ? 1 : -1;
        if (jb.chain) { q.A = qsize - 1 - qs0; q.B = -step; } else { q.A = qs0; q.B = step; }
        t.A = right ? jb.sstart : jb.sstart - 1; t.B = step;
        if (right) { query_size = qsize - jb.qstart; target_size = tsize - jb.sstart; }
        else { query_size = jb.qstart; target_size = jb.sstart; }
        // a start point in front of a read (the reference's wrapped `short` seed numbers give a read beyond 327 670 bases negative query
        // starts, pw_impl.cpp:388; there the reference extends from in front of its buffer): nothing to extend here
        if (jb.qstart < 0 || jb.sstart < 0) { query_size = 0; target_size = 0; }
        while (true) {
            // retrieve_next_aln_block (gapalign.cpp:9-45)
            const int qleft = query_size - qidx, tleft = target_size - tidx;
            int qblk, tblk, last_block;
            if (qleft < SEG_BLK + 100 || tleft < SEG_BLK + 100) {
                qblk = min(qleft, (int)(tleft + tleft * 0.2));
                tblk = min(tleft, (int)(qleft + qleft * 0.2));
                last_block = 1;
            } else { qblk = SEG_BLK; tblk = SEG_BLK; last_block = 0; }
            if (qblk < 0) qblk = 0;
            if (tblk < 0) tblk = 0;
            __builtin_amdgcn_wave_barrier();
            if (lane < SEQ_WORDS) {     // word 0 is the pad word, word 1 + j holds logical bases 16j .. 16j+15
                S.Qp[lane] = (lane > 0 && (lane - 1) * 16 < qblk + 32) ? view_word(q, qidx + (lane - 1) * 16) : 0u;
                S.Tp[lane] = (lane > 0 && (lane - 1) * 16 < tblk + 32) ? view_word(t, tidx + (lane - 1) * 16) : 0u;
            }
            __builtin_amdgcn_wave_barrier();
            BlockOut o;
            align_block<false>(S, qblk, tblk, grow, o, ucells, usnake, st);
            if (o.fallback) { ++nfallback; align_block<true>(S, qblk, tblk, grow, o, ucells, usnake, st); }
            ++nblocks;
            R.blocks += 1;
            if (!o.aligned_or_best || !o.trim_ok) break;
            const int full_map = (qblk - o.qe <= 20 || tblk - o.te <= 20);
            int qcnt = o.qcnt, tcnt = o.tcnt, acnt = o.acnt;
            if (last_block || !full_map) { qcnt -= 4; tcnt -= 4; acnt -= 4; }
            const int cols = (o.qe + o.te + o.dist) / 2 - acnt;
            const int mcut = qcnt + tcnt - acnt;
            R.columns += cols;
            R.matches += (o.qe + o.te - o.dist) / 2 - mcut;
            R.qbases += o.qe - qcnt;
            R.tbases += o.te - tcnt;
            if (last_block || !full_map) break;
            qidx += o.qe - qcnt;
            tidx += o.te - tcnt;
        }
        if (lane == 0) dres[unit] = R;
        cells += ucells; snake += usnake;
        ucells = 0; usnake = 0;
    }
    // snake bases are counted per lane
    for (int off = 32; off > 0; off >>= 1) snake += __shfl_xor(snake, off);
    if (lane == 0) {
        atomicAdd(&counters[3], nblocks);
        atomicAdd(&counters[4], cells);
        atomicAdd(&counters[5], snake);
        atomicAdd(&counters[8], nfallback);       // debug slots: blocks re-run with spilled rows, rows, fast rows, wide rows, unaligned blocks
        atomicAdd(&counters[9], (unsigned long long)st.rows);
        atomicAdd(&counters[10], (unsigned long long)st.fast_rows);
        atomicAdd(&counters[11], (unsigned long long)st.wide_rows);
        atomicAdd(&counters[12], (unsigned long long)st.unaligned);
    }
}

int dw_extend_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, DirResult* dres,
                     const DwHandover* hand, const unsigned int* hand_count, unsigned int* cursor) {
    int waves_per_cu = 16;                              // 4 waves per SIMD (VGPR budget); LDS 9.2 KB per wave
    if (const char* e = getenv("MECAT_DW_WAVES")) waves_per_cu = std::max(4, std::min(32, atoi(e)));   // tuning/debug knob
    const int max_waves = c->num_cus * waves_per_cu;
    const int grid = std::min(max_waves / AL_WAVES, (2 * n + AL_WAVES - 1) / AL_WAVES);
    uint16_t* d_g;                                      // the spilled rows of a re-run block, per wave
    if (c->scratch("al_rows", sizeof(uint16_t) * GROW_STRIDE * (size_t)max_waves, (void**)&d_g)) return -1;
    LAUNCH(c, "dw_extend", dw_extend, grid, AL_BLOCK, 0, (const uint32_t*)ref->d_pac, (const mhip_offset_t*)ref->d_offs,
           (const uint32_t*)reads->d_pac, (const mhip_offset_t*)reads->d_offs, (const mhip_aln_job*)d_jobs, n, dres, d_g, cursor,
           (unsigned long long*)c->d_counters, hand, hand_count);
    return 0;
}
