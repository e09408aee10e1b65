// ref_extend.hip — mecat2ref, stage 2: every listed candidate through DiffAligner::go on the device, with the two
// aligned strings as 2-bit columns.  PacBio mode (the tool's default `-x 0`); in nanopore mode the same jobs, bounds, slices, stitch and
// join run around ref_xextend.hip's kernel (ref_extend_run's `aligner`).
//
// Replaces the extend_candidate loop of reference_mapping (mecat2ref/mecat2ref_impl_large.cpp:566-582 for round 1, :829-845 for round 2):
//   extend_candidate         mecat2ref/mecat2ref_aux.cpp:123-183    the job, go, the result's coordinates
//   extract_sequences        mecat2ref/mecat2ref_aux.cpp:85-121     the window of the concatenated reference, the read's codes
//   DiffAligner::go          common/diff_gapalign.cpp:294-349       left + right extension from the seed point, stitching
//   dw_in_one_direction      common/diff_gapalign.cpp:221-292       block chaining with the 4-match tail anchor
//   retrieve_next_aln_block  common/gapalign.cpp:9-45               500-bp blocks, last-block sizing
//   Align                    common/diff_gapalign.cpp:107-219       O(ND) wavefront with the adaptive band, best-point fallback
//   GetAlignString           common/diff_gapalign.cpp:39-104        traceback
//   trim_mismatch_end        common/gapalign.cpp:47-68              tail anchor
// The rules are dw_extend.hip's (same reference lines); what differs is what is kept: every block keeps all its d-rows, the whole path is
// traced, and each direction comes out as 2-bit columns in extension order: 0 = both bases (O(ND) paths have no mismatch columns),
// 1 = target base only ('-' in the query string), 2 = query base only.
//
// Kernels, in call order:
//   ref_jobs     one job per slot of the candidate lists ([n][maxc] + counts, mhip_ref_seed_reads' layout) with extract_sequences'
//                arithmetic, and each direction's column bound (its query bases + its window bases) in 32-bit words
//   ref_scan     the bounds -> each direction's place in the column store (scan.h); the ok results' words -> their place in the dense output
//   ref_extend   one wave per (job, direction), lanes = the diagonals of a d-row, persistent waves on an atomic cursor (dw_extend's mapping).
//                The target is staged from the reference volume by ABSOLUTE base position (ref_genome.cpp's volume has no pad bases and
//                stores every letter that is not A, C, G, T as code 0: the tool's `if (c > 3) c = 0`), the query from the reads volume by
//                read and strand.  The strand rule is the tool's: reference_mapping reverses the whole read and complements only upper-case
//                A, C, G, T (:376-410), and extract_sequences encodes with a table that knows lower case — so on the reverse strand a base
//                whose N-plane entry is set keeps its stored code and every other base is complemented (ref_reads.h packs reads that way).
//   ref_stitch   go's coordinates (:309-346), sb / se, ok = columns >= 1000, the words an ok result takes
//   ref_join     an ok result's columns in STRING order: the left direction reversed, then the right one
// A call whose worst-case column store exceeds the budget (a quarter of the free device memory; MECAT_REF_COLS_BUDGET, in words, read at
// call time) is cut into slices of jobs; a slice's dense words then leave the device at the end of the slice.
//
// LDS per wave: RxLds = 5 584 bytes (blocks 416, V / path 1 616, band limits 1 600, window 1 152, row offsets 800) -> 28 waves per CU by
// LDS; the launch keeps dw_extend's 16 waves per CU (4 per SIMD).  Rows go to a per-wave global scratch of RX_GROW cells ("rx_rows") and
// come back a window at a time for the walk, as in cns_extend.hip.  Nothing here is tuned yet: see profiles/ref_extend.md.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "dw_helpers.h"
#include "ref_extend.h"
#include "scan.h"

#define RX_BLOCK 256
#define RX_WAVES (RX_BLOCK / WAVE)
#define RX_SEG 500               // DiffAlignParameters::segment_size, diff_gapalign.h:35
#define RX_MAX_BLK 736           // last block (gapalign.cpp:24-30): one side < 600, the other <= int(599 * 1.2) = 718
#define RX_SEQ_WORDS 52          // 736 / 16 = 46 words + the pad word + window slack
#define RX_MAX_D 400             // int(0.3 * (599 + 718)) = 395
#define RX_VLEN (2 * RX_MAX_D + 8)
#define RX_ROW_W 224             // diagonals per d-row: (2 * int(0.3 * 718)) / 2 + 1 = 216, + the two the band grows by
#define RX_RING 512              // cells of the walk's row window; >= RX_MAX_D (reused per row) and >= a row
#define RX_GROW ((size_t)RX_MAX_D * RX_ROW_W)
#define RX_RM 100000             // the tool's read buffers (RM, mecat2ref_defs.h)
#define RX_MIN_COLS 1000         // extend_candidate's min_aln_size (mecat2ref_aux.cpp:152)

struct RxLds {
    uint32_t Qp[RX_SEQ_WORDS];
    uint32_t Tp[RX_SEQ_WORDS];
    union {
        int16_t V[RX_VLEN];        // forward rows
        uint16_t tlen[RX_MAX_D];   // afterwards, the path: snake length of the row, bit 15 = the row's indel is a query-only column
    };
    int16_t rmin[RX_MAX_D], rmax[RX_MAX_D];
    uint16_t woff[64];             // walk: offset of row r in the window, at r mod 64
    uint16_t ring[RX_RING];        // the row window; after the walk: columns before row r's snake, at r
    uint16_t roff[RX_MAX_D];       // where row d starts in the wave's global scratch, in pairs of cells
};
static_assert(RX_RING >= RX_MAX_D && RX_RING >= RX_ROW_W, "the ring holds a row and doubles as the per-row column prefix");
static_assert(RX_GROW / 2 < 65536, "row offsets in pairs of cells fit 16 bits");

namespace {

// ---------------------------------------------------------------- jobs and bounds
// extract_sequences' arithmetic (mecat2ref_aux.cpp:97-101) per slot; words[2 s + d] = the 32-bit words direction d's columns can take.
// err[0] is set when a listed candidate starts outside the reference or the read (or a count is no list length): nothing is extended then.
__global__ __launch_bounds__(256) void ref_jobs(const mhip_ref_candidate* __restrict__ cands, const int32_t* __restrict__ counts, int n, int maxc,
                                                int rid_begin, const mhip_offset_t* __restrict__ qoffs, int64_t ref_size, RxJob* __restrict__ jobs,
                                                uint32_t* __restrict__ words, int* __restrict__ err) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n * maxc) return;
    const int i = s / maxc, k = s - i * maxc;
    RxJob j = {0, rid_begin + i, 0, 0, 0, 0, 0, 0, 0};
    const int cnt = counts[i];
    uint32_t wl = 0, wr = 0;
    if (cnt < 0 || cnt > maxc) {
        if (k == 0) atomicExch(err, 1);
    } else if (k < cnt) {
        const mhip_ref_candidate c = cands[s];
        const int64_t read_len = qoffs[rid_begin + i].size;
        const int64_t ref_start = c.loc1 - 1, read_start = c.loc2;
        if (ref_start < 0 || ref_start >= ref_size || read_start < 0 || read_start >= read_len || (c.chain != 0 && c.chain != 1)) atomicExch(err, 1);
        else {
            const int64_t L1 = read_start, R1 = read_len - read_start, L2 = ref_start, R2 = ref_size - ref_start;
            const int64_t L = L1 < L2 ? L1 : L2, R = R1 < R2 ? R1 : R2;
            const int64_t l12 = (int64_t)((double)L * 1.2), r12 = (int64_t)((double)R * 1.2);      // the product in double, truncated (:100-101)
            j.ref_start = ref_start;
            j.chain = c.chain; j.read_start = (int32_t)read_start; j.read_len = (int32_t)read_len;
            j.left = (int32_t)(L2 < l12 ? L2 : l12);
            j.right = (int32_t)(R2 < r12 ? R2 : r12);
            j.valid = 1; j.score = c.score;
            wl = (uint32_t)((j.read_start + j.left + 15) >> 4);
            wr = (uint32_t)((j.read_len - j.read_start + j.right + 15) >> 4);
        }
    }
    jobs[s] = j;
    words[2 * s] = wl;
    words[2 * s + 1] = wr;
}

// out[i] = base + in[0] + .. + in[i - 1] for i <= m (m + 1 values: the last one is the total)
__global__ __launch_bounds__(1024) void ref_scan(const uint32_t* __restrict__ in, long long m, unsigned long long base, unsigned long long* __restrict__ out) {
    const unsigned long long tot = scan_array_1024<unsigned long long>(m, base, [&](long long i) { return in[i]; },
                                                                       [&](long long i, unsigned long long v) { out[i] = v; });
    if (threadIdx.x == 0) out[m] = tot;
}

// ---------------------------------------------------------------- the extension
__device__ __forceinline__ int rx_cell(const RxLds& S, int r, int k) {
    return (int)S.ring[(int)S.woff[r & 63] + ((k - (int)S.rmin[r]) >> 1)];
}

// rows in the window ending at row r (going down): as many of r, r - 1, ... (at most 64) as fit RX_RING cells; the rows lie back to back
// in the global scratch, so the window is one contiguous range (cns_extend.hip's scheme).  Sets woff[]; returns the lowest row loaded.
__device__ __forceinline__ int rx_load_window(RxLds& S, const uint16_t* grow, int r, int lane) {
    const int ns_r = (((int)S.rmax[r] - (int)S.rmin[r]) >> 1) + 1;
    const int end = 2 * (int)S.roff[r] + ns_r;
    const int rr = r - lane;
    const int start = rr >= 0 ? 2 * (int)S.roff[rr] : 0;
    const unsigned long long fits = __ballot(rr >= 0 && end - start <= RX_RING);
    const int count = __popcll(fits);                      // a prefix of the lanes (start decreases with the lane); >= 1 (a row fits the ring)
    const int base = 2 * (int)S.roff[r - count + 1];
    if (lane < count) S.woff[rr & 63] = (uint16_t)(start - base);
    const int words = (end - base + 1) >> 1;               // <= RX_RING / 2
    const uint32_t* g32 = (const uint32_t*)grow + (base >> 1);
    constexpr int NW = RX_RING / 2 / 64;
    uint32_t v[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) v[j] = lane + 64 * j < words ? __hip_atomic_load(g32 + lane + 64 * j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
    for (int j = 0; j < NW; ++j)
        if (lane + 64 * j < words) ((uint32_t*)S.ring)[lane + 64 * j] = v[j];
    return r - count + 1;
}

// units [u0, u1) (unit = 2 * slot + direction, 0 = left); the columns of unit u start at word dbase[u] - dbase[u0] of dstore (zero-filled)
__global__ __launch_bounds__(RX_BLOCK, 4) void ref_extend(const uint32_t* __restrict__ rpac, const uint32_t* __restrict__ qpac,
                                                          const uint32_t* __restrict__ qnpac, const mhip_offset_t* __restrict__ qoffs,
                                                          const RxJob* __restrict__ jobs, unsigned int u0, unsigned int u1,
                                                          const unsigned long long* __restrict__ dbase, uint32_t* __restrict__ dstore,
                                                          RxDir* __restrict__ dres, uint16_t* __restrict__ gscratch, unsigned int* __restrict__ cursor,
                                                          unsigned long long* __restrict__ counters) {
    __shared__ RxLds lds[RX_WAVES];
    RxLds& S = lds[threadIdx.x >> 6];
    const int lane = lane_id();
    uint16_t* grow = gscratch + (size_t)(blockIdx.x * RX_WAVES + (threadIdx.x >> 6)) * RX_GROW;
    const unsigned long long base0 = dbase[u0];
    unsigned long long nblocks = 0;
    while (true) {
        unsigned int unit = 0;
        if (lane == 0) unit = atomicAdd(cursor, 1u);
        unit = __shfl(unit, 0) + u0;
        if (unit >= u1) break;
        const RxJob jb = jobs[unit >> 1];
        const int right = unit & 1;
        RxDir R = {0, 0, 0, 0};
        if (!jb.valid) { if (lane == 0) dres[unit] = R; continue; }
        // extension views: logical position i of the query is strand position read_start + i (right) or read_start - 1 - i (left); strand
        // position p of the reverse strand is original index read_len - 1 - p; the target is the concatenated reference itself
        SeqView q, t, qn;
        const int qs0 = right ? jb.read_start : jb.read_start - 1, step = right ? 1 : -1;
        q.pac = qpac; q.off = qoffs[jb.rid].offset; q.comp = jb.chain;
        if (jb.chain) { q.A = jb.read_len - 1 - qs0; q.B = -step; } else { q.A = qs0; q.B = step; }
        qn = q; qn.pac = qnpac; qn.comp = 0;
        t.pac = rpac; t.off = right ? jb.ref_start : jb.ref_start - 1; t.A = 0; t.B = step; t.comp = 0;
        const int query_size = right ? jb.read_len - jb.read_start : jb.read_start;
        const int target_size = right ? jb.right : jb.left;
        uint32_t* uops = dstore + (size_t)(dbase[unit] - base0);
        int qidx = 0, tidx = 0, cols = 0;
        while (true) {
            // retrieve_next_aln_block (gapalign.cpp:9-45)
            const int qleft = query_size - qidx, tleft = target_size - tidx;
            int q_len, t_len, last_block;
            if (qleft < RX_SEG + 100 || tleft < RX_SEG + 100) {
                q_len = min(qleft, (int)(tleft + tleft * 0.2));
                t_len = min(tleft, (int)(qleft + qleft * 0.2));
                last_block = 1;
            } else { q_len = RX_SEG; t_len = RX_SEG; last_block = 0; }
            const int band_tol = (int)(0.3 * (q_len > t_len ? q_len : t_len));      // dw_in_one_direction passes 0.3 * max(qblk, tblk) (:250)
            const int max_d = (int)(.3 * (q_len + t_len));                            // :122
            const int koff = max_d, band_size = band_tol * 2;
            __builtin_amdgcn_wave_barrier();
            if (lane < RX_SEQ_WORDS) {     // word 0 is the pad word, word 1 + j holds logical bases 16 j .. 16 j + 15
                const bool inq = lane > 0 && (lane - 1) * 16 < q_len + 32, intt = lane > 0 && (lane - 1) * 16 < t_len + 32;
                uint32_t w = inq ? view_word(q, qidx + (lane - 1) * 16) : 0u;
                if (inq && qnpac && q.comp) w = unflip_symbols(w, view_word(qn, qidx + (lane - 1) * 16));
                S.Qp[lane] = w;
                S.Tp[lane] = intt ? view_word(t, tidx + (lane - 1) * 16) : 0u;
            }
            for (int i = lane; i < 2 * max_d + 4 && i < RX_VLEN; i += 64) S.V[i] = 0;     // V is zero-filled per block (:232-233)
            __builtin_amdgcn_wave_barrier();

            // ---- Align, forward rows (:132-195)
            int best_m = -1, best_x = -1, best_d = 0, best_k = 0, min_k = 0, max_k = 0;
            int end_d = -1, end_k = 0, end_x = 0;
            int cum = 0;                                 // cells of the rows written so far (every row padded to an even length)
            for (int d = 0; d < max_d; ++d) {
                if (max_k - min_k > band_size) break;
                const int nslot = ((max_k - min_k) >> 1) + 1;
                if (lane == 0) { S.rmin[d] = (int16_t)min_k; S.rmax[d] = (int16_t)max_k; S.roff[d] = (uint16_t)(cum >> 1); }
                int bkey = -1, hkey = 0x7fffffff;
                constexpr int MAXJ = (RX_ROW_W + 63) / 64;
                int us[MAXJ];
                const int NJ = (nslot + 63) >> 6;
#pragma unroll
                for (int j = 0; j < MAXJ; ++j) {
                    us[j] = -0x40000000;
                    if (j >= NJ) continue;
                    const int tt = lane + 64 * j;
                    const bool act = tt < nslot;
                    const int k = min_k + 2 * tt, kk = k + koff;
                    const int16_t* vp = &S.V[act ? kk - 1 : 0];
                    const int vl = vp[0], vr = vp[2];
                    int x = (k == min_k || (k != max_k && vl < vr)) ? vr : vl + 1;       // :138-141
                    x = act ? x : q_len;
                    int y = act ? x - k : 0;
                    bool again;
                    do {
                        const int lim = min(q_len - x, t_len - y);
                        const int m = min(match16(S.Qp, min(x, RX_MAX_BLK), S.Tp, min(y, RX_MAX_BLK)), lim);
                        const int nn = min(m, 16);
                        x += nn; y += nn;
                        again = m > 16;
                    } while (__ballot(again));
                    us[j] = act ? x + y : -0x40000000;
                    if (act) {
                        grow[cum + tt] = (uint16_t)x;
                        bkey = max(bkey, ((x + y) << 10) | (1023 - kk));                      // first maximum of x + y in k order (:160-167)
                        if (x >= q_len || y >= t_len) hkey = min(hkey, (kk << 10) | x);       // lowest diagonal first (:168-169)
                    }
                }
                __builtin_amdgcn_wave_barrier();
                // V is updated after every diagonal of the row has read its neighbours (they have the other parity anyway)
#pragma unroll
                for (int j = 0; j < MAXJ; ++j) {
                    const int tt = lane + 64 * j;
                    if (tt < nslot) { const int k = min_k + 2 * tt; S.V[k + koff] = (int16_t)((us[j] + k) >> 1); }
                }
                cum += (nslot + 1) & ~1;
                bkey = wave_max(bkey);
                {
                    const int rm = bkey >> 10, rk = 1023 - (bkey & 1023) - koff;
                    if (rm > best_m) { best_m = rm; best_x = (rm + rk) / 2; best_d = d; best_k = rk; }
                }
                if (__ballot(hkey != 0x7fffffff)) {      // some diagonal reached an end: the lowest one ends the block
                    hkey = wave_min(hkey);
                    end_d = d; end_k = (hkey >> 10) - koff; end_x = hkey & 1023;
                    break;
                }
                // band (:172-179): first / last diagonal within band_tol of the best
                int nmin = max_k, nmax = min_k;
                {
                    int first = -1, last = -1;
#pragma unroll
                    for (int j = 0; j < MAXJ; ++j) {
                        if (j >= NJ) continue;
                        const unsigned long long qb = __ballot(lane + 64 * j < nslot && us[j] >= best_m - band_tol);
                        if (qb) {
                            if (first < 0) first = 64 * j + __builtin_ctzll(qb);
                            last = 64 * j + 63 - __builtin_clzll(qb);
                        }
                    }
                    if (first >= 0) { nmin = min_k + 2 * first; nmax = min_k + 2 * last; }
                }
                max_k = nmax + 1;
                min_k = nmin - 1;
                __builtin_amdgcn_wave_barrier();
            }
            ++nblocks;
            R.blocks += 1;
            if (end_d < 0) {                             // no end reached: the best point, if any (:197-215)
                if (best_x > 0) { end_d = best_d; end_k = best_k; end_x = best_x; }
                else break;                              // aln_str_size 0: trim_mismatch_end fails
            }
            const int end_y = end_x - end_k;

            // ---- the path, end to start (GetAlignString :48-64): one scalar walk, every lane the same.  Row cd needs its two neighbours
            // in row cd - 1 (always inside that row's band: DESIGN.md); the rows come back from the global scratch a window at a time.
            __threadfence();
            __builtin_amdgcn_wave_barrier();
            int rstar = -1, x2s = 0, ks = 0;             // the last row (highest d) whose snake has >= 4 matches
            {
                int ck = end_k, x2 = end_x, w_lo = end_d;        // rows [w_lo, ...] are in the window
                for (int cd = end_d; cd >= 0; --cd) {
                    int x1 = 0, pre = ck, px2 = 0;
                    if (cd > 0) {
                        if (cd - 1 < w_lo) {
                            __builtin_amdgcn_wave_barrier();
                            w_lo = rx_load_window(S, grow, cd - 1, lane);
                            __builtin_amdgcn_wave_barrier();
                        }
                        const int cmin = S.rmin[cd], cmax = S.rmax[cd], pmin = S.rmin[cd - 1], pmax = S.rmax[cd - 1];
                        const int kl = ck - 1, kr = ck + 1;
                        const int vl = (kl >= pmin && kl <= pmax) ? rx_cell(S, cd - 1, kl) : 0;
                        const int vr = (kr >= pmin && kr <= pmax) ? rx_cell(S, cd - 1, kr) : 0;
                        if (ck == cmin || (ck != cmax && vl < vr)) { pre = kr; x1 = vr; px2 = vr; }
                        else { pre = kl; x1 = vl + 1; px2 = vl; }
                    }
                    const int len = x2 - x1;
                    if (rstar < 0 && len >= 4) { rstar = cd; x2s = x2; ks = ck; }
                    if (lane == 0) S.tlen[cd] = (uint16_t)(len | (cd > 0 && ck > pre ? 0x8000 : 0));   // from k - 1: query base only
                    ck = pre;
                    x2 = px2;
                }
            }
            __builtin_amdgcn_wave_barrier();

            // ---- columns before each row's snake
            int carry = 0;
            for (int r0 = 0; r0 <= end_d; r0 += 64) {
                const int r = r0 + lane;
                const bool in = r <= end_d;
                const int len = in ? (int)(S.tlen[r] & 0x7FFF) : 0;
                int incl = len + (in && r > 0 ? 1 : 0);          // the row's indel column + its snake
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(incl, o);
                    if (lane >= o) incl += v;
                }
                if (in) S.ring[r] = (uint16_t)(carry + incl - len);     // columns before the snake of row r (its indel included)
                carry += __shfl(incl, 63);
            }
            __builtin_amdgcn_wave_barrier();
            const int ncols = carry;                     // == (end_x + end_y + end_d) / 2: the path starts at (0, 0)

            // ---- trim_mismatch_end(.., 4, ..) (gapalign.cpp:47-68): back to the end of the last run of four matches
            if (rstar < 0) break;
            int acnt = ncols - ((int)S.ring[rstar] + (int)(S.tlen[rstar] & 0x7FFF)) + 4;
            int qcnt = end_x - x2s + 4, tcnt = end_y - (x2s - ks) + 4;
            if (ncols - acnt < 2) break;                 // "m == mat_cnt && k > 0"
            const int full_map = (q_len - end_x <= 20 || t_len - end_y <= 20);        // :269-270
            if (last_block || !full_map) { qcnt -= 4; tcnt -= 4; acnt -= 4; }
            const int kept_cols = ncols - acnt;
            // ---- emit: 0 = both bases (the store is zero-filled), 1 = target base only, 2 = query base only
            for (int r0 = 1; r0 <= end_d; r0 += 64) {
                const int r = r0 + lane;
                const bool in = r <= end_d;
                const int c = in ? (int)S.ring[r] - 1 : 0x7fffffff;          // column of the row's indel
                if (in && c < kept_cols) {
                    const int gc = cols + c;
                    atomicOr(&uops[gc >> 4], (uint32_t)((S.tlen[r] & 0x8000) ? 2 : 1) << ((gc & 15) << 1));
                }
            }
            cols += kept_cols;
            R.qbases += end_x - qcnt;
            R.tbases += end_y - tcnt;
            if (last_block || !full_map) break;
            qidx += end_x - qcnt;
            tidx += end_y - tcnt;
        }
        R.cols = cols;
        if (lane == 0) dres[unit] = R;
    }
    if (lane == 0) atomicAdd(&counters[3], nblocks);
}

// ---------------------------------------------------------------- stitch and join
// go's coordinates (:324-325, :343-344), extend_candidate's sb / se (:161-162); words[s] = the words result s takes in the dense output
// xdrop: XdropAligner::go's rule (xdrop_gapalign.cpp:438), ok = the query span >= 1000, not the columns; cols = aln_size either way
__global__ __launch_bounds__(256) void ref_stitch(const RxJob* __restrict__ jobs, const RxDir* __restrict__ dres, int s0, int s1, int xdrop,
                                                  mhip_ref_result* __restrict__ res, uint32_t* __restrict__ words,
                                                  unsigned long long* __restrict__ counters) {
    const int s = s0 + blockIdx.x * 256 + threadIdx.x;
    if (s >= s1) return;
    const RxJob j = jobs[s];
    mhip_ref_result r = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t w = 0;
    if (j.valid) {
        const RxDir L = dres[2 * s], R = dres[2 * s + 1];
        r.cols = L.cols + R.cols;
        r.chain = j.chain; r.vscore = j.score;
        r.qb = j.read_start - L.qbases; r.qe = j.read_start + R.qbases; r.qs = j.read_len;
        r.ok = xdrop ? r.qe - r.qb >= RX_MIN_COLS : r.cols >= RX_MIN_COLS;
        r.sb = j.ref_start - L.tbases; r.se = j.ref_start + R.tbases;      // ref_start - left + (left -/+ bases)
        w = r.ok ? (uint32_t)((r.cols + 15) >> 4) : 0u;
        if (r.ok) {                                  // the work counters dw_stitch keeps (align.hip)
            atomicAdd(&counters[6], (unsigned long long)(r.qe - r.qb));
            atomicAdd(&counters[7], 1ull);
        }
    }
    res[s] = r;
    words[s - s0] = w;
}

__device__ __forceinline__ uint32_t rx_col(const uint32_t* p, int c) { return (p[c >> 4] >> ((c & 15) << 1)) & 3u; }

// one thread per output word: column c of the string is left column lcols - 1 - c, or right column c - lcols
__global__ __launch_bounds__(256) void ref_join(const mhip_ref_result* __restrict__ res, const RxDir* __restrict__ dres, int s0, int s1,
                                                const unsigned long long* __restrict__ dbase, unsigned int u0, const uint32_t* __restrict__ dstore,
                                                const unsigned long long* __restrict__ woffs /* of the slice: [s - s0] */, unsigned long long wbase,
                                                uint32_t* __restrict__ dense) {
    const int s = s0 + blockIdx.x;
    if (s >= s1 || !res[s].ok) return;
    const int lcols = dres[2 * s].cols, cols = res[s].cols;
    const uint32_t* lp = dstore + (size_t)(dbase[2 * s] - dbase[u0]);
    const uint32_t* rp = dstore + (size_t)(dbase[2 * s + 1] - dbase[u0]);
    uint32_t* out = dense + (size_t)(woffs[s - s0] - wbase);
    for (int w = threadIdx.x; w < (cols + 15) >> 4; w += 256) {
        uint32_t v = 0;
        for (int b = 0; b < 16; ++b) {
            const int c = 16 * w + b;
            if (c < cols) v |= (c < lcols ? rx_col(lp, lcols - 1 - c) : rx_col(rp, c - lcols)) << (b << 1);
        }
        out[w] = v;
    }
}

int64_t g_last_stats[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};      // of the last run into each buffer set: jobs, slices, bytes of row scratch, words of the column store
int64_t g_last_xstats[4] = {0, 0, 0, 0};                         // of the last X-drop run into set 0: jobs, slices, blocks redone with the wide block, words of the column store

}  // namespace

// Results, word offsets and dense words go to buffer set `set` (ref_extend.h) and stay there until the next run into the same set;
// everything else is working memory shared by the sets.
int ref_extend_run(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc, int aligner,
                   const mhip_ref_candidate* d_cands, const int32_t* d_counts, int64_t* total_words, int set) {
    c->rx_slots[set] = 0; c->rx_total[set] = 0; c->rx_on_host[set] = false;
    if (total_words) *total_words = 0;
    if (aligner != RX_ALIGNER_DIFF && aligner != RX_ALIGNER_XDROP) { mhip_set_error("mhip_ref_extend_run: aligner %d", aligner); return -1; }
    const bool xdrop = aligner == RX_ALIGNER_XDROP;
    if (xdrop && set == 0) for (int i = 0; i < 4; ++i) g_last_xstats[i] = 0;
    if (rid_begin < 0 || rid_end < rid_begin || rid_end > reads->num_reads) { mhip_set_error("mhip_ref_extend_run: bad read range [%d, %d) of %d", rid_begin, rid_end, reads->num_reads); return -1; }
    if (maxc < 1 || maxc > 100) { mhip_set_error("mhip_ref_extend_run: list length %d outside [1, 100]", maxc); return -1; }
    for (int r = rid_begin; r < rid_end; ++r)
        if (reads->h_offs[r].size >= RX_RM) {
            mhip_set_error("mhip_ref_extend_run: read %d has %d letters; mecat2ref's read buffers hold fewer than %d", r, reads->h_offs[r].size, RX_RM);
            return -1;
        }
    const int n = rid_end - rid_begin;
    for (int i = 0; i < 4; ++i) g_last_stats[set][i] = 0;
    if (n == 0) return 0;
    const int slots = n * maxc;
    const long long units = 2ll * slots;
    RxJob* d_jobs;
    uint32_t *d_words, *d_rwords;
    unsigned long long *d_dbase, *d_woffs, *d_swoffs;
    RxDir* d_dres;
    mhip_ref_result* d_res;
    unsigned int* d_cur;
    if (c->scratch("rx_jobs", sizeof(RxJob) * (size_t)slots, (void**)&d_jobs)) return -1;
    if (c->scratch("rx_words", sizeof(uint32_t) * (size_t)units, (void**)&d_words)) return -1;
    if (c->scratch("rx_rwords", sizeof(uint32_t) * (size_t)slots, (void**)&d_rwords)) return -1;
    if (c->scratch("rx_dbase", sizeof(unsigned long long) * (size_t)(units + 1), (void**)&d_dbase)) return -1;
    if (scratch_set(c, "rx_woffs", set, sizeof(unsigned long long) * (size_t)(slots + 1), (void**)&d_woffs)) return -1;
    if (c->scratch("rx_swoffs", sizeof(unsigned long long) * (size_t)(slots + 1), (void**)&d_swoffs)) return -1;
    if (c->scratch("rx_dres", sizeof(RxDir) * (size_t)units, (void**)&d_dres)) return -1;
    if (scratch_set(c, "rx_res", set, sizeof(mhip_ref_result) * (size_t)slots, (void**)&d_res)) return -1;
    if (c->scratch("rx_cursor", 64, (void**)&d_cur)) return -1;
    HIPCHK(hipMemsetAsync(d_cur, 0, 64, c->stream));
    LAUNCH(c, "ref_jobs", ref_jobs, (slots + 255) / 256, 256, 0, d_cands, d_counts, n, maxc, rid_begin, (const mhip_offset_t*)reads->d_offs,
           (int64_t)ref->num_bases, d_jobs, d_words, (int*)(d_cur + 8));
    LAUNCH(c, "ref_scan", ref_scan, 1, 1024, 0, (const uint32_t*)d_words, units, 0ull, d_dbase);
    HIPCHK(hipGetLastError());
    unsigned int st[16];
    unsigned long long cap_total = 0;
    HIPCHK(hipMemcpyAsync(st, d_cur, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&cap_total, d_dbase + units, sizeof(cap_total), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (st[8]) {
        mhip_set_error("mhip_ref_extend_run: a candidate starts outside the reference or its read (or a list count is outside [0, %d]): nothing extended", maxc);
        return -1;
    }
    // ---- slices of jobs whose worst-case columns fit the budget
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    unsigned long long budget = std::max<unsigned long long>(1, free_b / 4 / sizeof(uint32_t));
    if (const char* e = getenv("MECAT_REF_COLS_BUDGET")) { if (atoll(e) > 0) budget = (unsigned long long)atoll(e); }
    std::vector<int> cuts = {0};                         // slice i = slots [cuts[i], cuts[i + 1])
    unsigned long long store_words = cap_total;
    if (cap_total > budget) {
        std::vector<unsigned long long> h_dbase((size_t)units + 1);
        HIPCHK(hipMemcpyAsync(h_dbase.data(), d_dbase, sizeof(unsigned long long) * h_dbase.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        store_words = 0;
        int first = 0;
        for (int s = 0; s < slots; ++s)                  // (a job larger than the budget is a slice of its own)
            if (s > first && h_dbase[2 * (size_t)s + 2] - h_dbase[2 * (size_t)first] > budget) {
                store_words = std::max(store_words, h_dbase[2 * (size_t)s] - h_dbase[2 * (size_t)first]);
                cuts.push_back(s);
                first = s;
            }
        store_words = std::max(store_words, h_dbase[(size_t)units] - h_dbase[2 * (size_t)first]);
    }
    cuts.push_back(slots);
    const int nslices = (int)cuts.size() - 1;
    uint32_t *d_store, *d_dense;
    if (c->scratch("rx_store", sizeof(uint32_t) * (size_t)(store_words + 1), (void**)&d_store)) return -1;
    // an ok result's words are no more than its two directions' bounds: the dense output of a slice fits what its store takes
    if (scratch_set(c, "rx_dense", set, sizeof(uint32_t) * (size_t)(store_words + 1), (void**)&d_dense)) return -1;
    const int max_waves = c->num_cus * 16;               // 4 waves per SIMD, as dw_extend; LDS 5.6 KB per wave
    uint16_t* d_g = nullptr;
    if (!xdrop && c->scratch("rx_rows", sizeof(uint16_t) * RX_GROW * (size_t)max_waves, (void**)&d_g)) return -1;
    g_last_stats[set][0] = slots; g_last_stats[set][1] = nslices; g_last_stats[set][2] = xdrop ? 0 : (int64_t)(sizeof(uint16_t) * RX_GROW * (size_t)max_waves);
    g_last_stats[set][3] = (int64_t)store_words;
    if (nslices > 1) c->rx_words[set].clear();
    unsigned long long wbase = 0;
    for (int i = 0; i < nslices; ++i) {
        const int s0 = cuts[(size_t)i], s1 = cuts[(size_t)i + 1];
        const unsigned int u0 = 2u * (unsigned)s0, u1 = 2u * (unsigned)s1;
        const int grid = std::max(1, std::min(max_waves / RX_WAVES, (int)((u1 - u0 + RX_WAVES - 1) / RX_WAVES)));
        HIPCHK(hipMemsetAsync(d_store, 0, sizeof(uint32_t) * (size_t)(store_words + 1), c->stream));
        HIPCHK(hipMemsetAsync(d_cur, 0, sizeof(unsigned int), c->stream));
        if (xdrop) {                                     // (d_cur + 12 counts the blocks redone with the wide block, over the slices)
            if (ref_xextend_launch(c, ref, reads, d_jobs, u0, u1, d_dbase, d_store, d_dres, d_cur, d_cur + 12)) return -1;
        } else
            LAUNCH(c, "ref_extend", ref_extend, grid, RX_BLOCK, 0, (const uint32_t*)ref->d_pac, (const uint32_t*)reads->d_pac, (const uint32_t*)reads->d_npac,
                   (const mhip_offset_t*)reads->d_offs, (const RxJob*)d_jobs, u0, u1, (const unsigned long long*)d_dbase, d_store, d_dres, d_g, d_cur,
                   (unsigned long long*)c->d_counters);
        LAUNCH(c, "ref_stitch", ref_stitch, (s1 - s0 + 255) / 256, 256, 0, (const RxJob*)d_jobs, (const RxDir*)d_dres, s0, s1, xdrop ? 1 : 0, d_res, d_rwords,
               (unsigned long long*)c->d_counters);
        LAUNCH(c, "ref_scan", ref_scan, 1, 1024, 0, (const uint32_t*)d_rwords, (long long)(s1 - s0), wbase, d_swoffs);
        LAUNCH(c, "ref_join", ref_join, s1 - s0, 256, 0, (const mhip_ref_result*)d_res, (const RxDir*)d_dres, s0, s1, (const unsigned long long*)d_dbase, u0,
               (const uint32_t*)d_store, (const unsigned long long*)d_swoffs, wbase, d_dense);
        HIPCHK(hipGetLastError());
        // the slice's offsets into the call's table (the entry behind the last slot is the running total)
        HIPCHK(hipMemcpyAsync(d_woffs + s0, d_swoffs, sizeof(unsigned long long) * (size_t)(s1 - s0 + 1), hipMemcpyDeviceToDevice, c->stream));
        unsigned long long wend = 0;
        HIPCHK(hipMemcpyAsync(&wend, d_swoffs + (s1 - s0), sizeof(wend), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (nslices > 1) {                               // the dense buffer is the next slice's: its words leave the device now
            c->rx_words[set].resize((size_t)wend);
            if (wend > wbase) HIPCHK(hipMemcpy(c->rx_words[set].data() + wbase, d_dense, sizeof(uint32_t) * (size_t)(wend - wbase), hipMemcpyDeviceToHost));
        }
        wbase = wend;
    }
    if (xdrop && set == 0) {
        unsigned int redone = 0;
        HIPCHK(hipMemcpy(&redone, d_cur + 12, sizeof(redone), hipMemcpyDeviceToHost));
        g_last_xstats[0] = slots; g_last_xstats[1] = nslices; g_last_xstats[2] = redone; g_last_xstats[3] = (int64_t)store_words;
    }
    c->rx_slots[set] = slots; c->rx_total[set] = (int64_t)wbase; c->rx_on_host[set] = nslices > 1;
    if (total_words) *total_words = (int64_t)wbase;
    return 0;
}

int ref_extend_fetch(mhip_ctx* c, int set, mhip_ref_result* res, uint64_t* word_offs, uint32_t* ops_dense) {
    const int slots = c->rx_slots[set];
    if (slots == 0) { if (word_offs) word_offs[0] = 0; return 0; }
    mhip_ref_result* d_res;
    unsigned long long* d_woffs;
    uint32_t* d_dense;
    if (scratch_set(c, "rx_res", set, 0, (void**)&d_res) || scratch_set(c, "rx_woffs", set, 0, (void**)&d_woffs) || scratch_set(c, "rx_dense", set, 0, (void**)&d_dense)) return -1;
    HIPCHK(hipMemcpyAsync(res, d_res, sizeof(mhip_ref_result) * (size_t)slots, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(word_offs, d_woffs, sizeof(uint64_t) * (size_t)(slots + 1), hipMemcpyDeviceToHost, c->stream));
    if (c->rx_total[set] > 0) {
        if (c->rx_on_host[set]) memcpy(ops_dense, c->rx_words[set].data(), sizeof(uint32_t) * (size_t)c->rx_total[set]);
        else HIPCHK(hipMemcpyAsync(ops_dense, d_dense, sizeof(uint32_t) * (size_t)c->rx_total[set], hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

namespace {

// a run on HOST lists: the lists go to the device, then ref_extend_run
int rx_run_host(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc, int aligner,
                const mhip_ref_candidate* cands, const int32_t* counts, int64_t* total_words) {
    const int n = rid_end - rid_begin;
    mhip_ref_candidate* d_c = nullptr;
    int32_t* d_n = nullptr;
    if (n > 0 && maxc >= 1 && maxc <= 100) {
        if (c->scratch("rx_in_cands", sizeof(mhip_ref_candidate) * (size_t)n * (size_t)maxc, (void**)&d_c)) return -1;
        if (c->scratch("rx_in_counts", sizeof(int32_t) * (size_t)n, (void**)&d_n)) return -1;
        HIPCHK(hipMemcpyAsync(d_c, cands, sizeof(mhip_ref_candidate) * (size_t)n * (size_t)maxc, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_n, counts, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));       // (the caller's arrays are read until here)
    }
    return ref_extend_run(c, ref, reads, rid_begin, rid_end, maxc, aligner, d_c, d_n, total_words, 0);
}

// the PacBio entry points keep refusing the other technology: nanopore mode has entry points of its own
int rx_refuse_tech(mhip_ctx* c, int tech) {
    if (tech == 0) return 0;
    c->rx_slots[0] = 0; c->rx_total[0] = 0; c->rx_on_host[0] = false;
    mhip_set_error("mhip_ref_extend_run: tech = %d: this call is PacBio mode (tech 0, DiffAligner); nanopore mode is mhip_ref_xextend_run", tech);
    return -1;
}

}  // namespace

extern "C" {

int mhip_ref_extend_run_dev(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc, int tech,
                            const mhip_ref_candidate* d_cands, const int32_t* d_counts, int64_t* total_words) {
    HIPCHK(hipSetDevice(c->device));
    if (rx_refuse_tech(c, tech)) return -1;
    return ref_extend_run(c, ref, reads, rid_begin, rid_end, maxc, RX_ALIGNER_DIFF, d_cands, d_counts, total_words, 0);
}

int mhip_ref_extend_run(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc, int tech,
                        const mhip_ref_candidate* cands, const int32_t* counts, int64_t* total_words) {
    HIPCHK(hipSetDevice(c->device));
    if (rx_refuse_tech(c, tech)) return -1;
    return rx_run_host(c, ref, reads, rid_begin, rid_end, maxc, RX_ALIGNER_DIFF, cands, counts, total_words);
}

int mhip_ref_xextend_run_dev(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc,
                             const mhip_ref_candidate* d_cands, const int32_t* d_counts, int64_t* total_words) {
    HIPCHK(hipSetDevice(c->device));
    return ref_extend_run(c, ref, reads, rid_begin, rid_end, maxc, RX_ALIGNER_XDROP, d_cands, d_counts, total_words, 0);
}

int mhip_ref_xextend_run(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc,
                         const mhip_ref_candidate* cands, const int32_t* counts, int64_t* total_words) {
    HIPCHK(hipSetDevice(c->device));
    return rx_run_host(c, ref, reads, rid_begin, rid_end, maxc, RX_ALIGNER_XDROP, cands, counts, total_words);
}

void mhip_ref_xextend_stats(int64_t out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = g_last_xstats[i];
}

int mhip_ref_extend_fetch(mhip_ctx* c, mhip_ref_result* res, uint64_t* word_offs, uint32_t* ops_dense) {
    HIPCHK(hipSetDevice(c->device));
    return ref_extend_fetch(c, 0, res, word_offs, ops_dense);
}

void mhip_ref_extend_stats(int64_t out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = g_last_stats[0][i];          // (set 0: the rescue's own extension does not show here)
}

}  // extern "C"
