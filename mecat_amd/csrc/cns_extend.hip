// cns_extend.hip — the one-unit O(ND) aligner that keeps the whole path: one wave per (candidate, direction), lanes are the diagonals
// of a d-row, 2 bits per alignment column out.
//
// Used for two things today.  cns_extend<false>: the units the mecat2cns forward pass (cns_forward = dw_extend2<true>, cns_fwd.h) hands
// over, about 0.2 % (MECAT_CNS_KERNEL=1 runs every unit through it; the tests compare the two).  cns_extend<true>: every unit of the
// mecat2asmpw / mecat2trimpw extension (asm_extend.hip).
//
// The rules are those of ns_banded_sw::Align / dw_in_one_direction of the reference's src/mecat2cns/dw.cpp (:146-375).  Same O(ND)
// core as the dw extension, different rules around it:
//   * max_d = int(2 * error_rate * (q_len + t_len)) (:163), square blocks: 500 x 500, or the rest when <= 600 (:322-326);
//   * no best-point fallback: a block that does not reach an end of its square ends the direction (:302-304, :333);
//   * the whole path is needed: the consensus stage consumes the aligned strings.  O(ND) paths have no mismatch columns,
//     so a column is one of {both bases, target base only, query base only}; the kernel emits 2 bits per column and the
//     host rebuilds "ACGT-" strings from the reads (cns_expand in hip.py / INTEGRATION.md);
//   * a block's tail is cut in front of its last run of four matches and the next block starts there (:336-351).
//
// Every row's furthest-x values go to a per-wave global scratch because the traceback walks all of them; the walk pulls them back
// into LDS a window of rows at a time (coalesced copies), which keeps the LDS footprint at 6.3 KB per wave = 24 waves per CU.
#include <algorithm>

#include "cns_defs.h"
#include "dw_helpers.h"

#define CN_BLOCK 256
#define CN_WAVES (CN_BLOCK / WAVE)
#define CN_MAXLEN 600              // a last block is at most CN_SEG + 100 bases per side
#define CN_VLEN (2 * CN_MAX_D + 8)
#define CN_ROW_W 192               // diagonals per row: band of 2 * int(0.3 * 600) = 360 -> 181 + 2
#define CN_SEQ_WORDS 44            // 600 bases + 32 of window slack = 40 words, one leading pad word, slack
#define CN_RING 512                // cells of the traceback's row window in LDS (~20 rows at 15 %); >= CN_MAX_D (reused per row below)
#define CN_GROW ((size_t)CN_MAX_D * CN_ROW_W)

struct CnsLds {
    uint32_t Qp[CN_SEQ_WORDS];
    uint32_t Tp[CN_SEQ_WORDS];
    union {
        int16_t V[CN_VLEN];        // forward rows
        uint16_t tlen[CN_MAX_D];   // afterwards, the path: snake length of the row, bit 15 = the row's indel is a query-only column
    };
    int16_t rmin[CN_MAX_D], rmax[CN_MAX_D];
    uint16_t woff[64];             // traceback: offset of row r in the window, at r mod 64 (a window holds <= 64 consecutive rows)
    uint16_t ring[CN_RING];        // the row window; after the walk: columns before row r's snake, at r
    uint16_t roff[CN_MAX_D];       // where row d starts in the wave's global scratch, in pairs of cells (rows are packed back to back, even length)
};

static_assert(CN_RING >= CN_MAX_D, "the ring doubles as the per-row column prefix");

__device__ __forceinline__ int cns_cell(const CnsLds& S, int r, int k) {
    return (int)S.ring[(int)S.woff[r & 63] + ((k - (int)S.rmin[r]) >> 1)];
}

// rows in the window ending at row r (going down): as many of r, r - 1, ... (at most 64) as fit CN_RING cells.  The rows lie
// back to back in the global scratch, so the window is one contiguous range: it is copied with full-wave 32-bit loads, all in
// flight at once (the rows were written by this wave: agent scope, past the L1).  Sets woff[]; returns the lowest row loaded.
__device__ __forceinline__ int cns_load_window(CnsLds& S, const uint16_t* grow, int r, int lane) {
    const int ns_r = S.rmax[r] >= S.rmin[r] ? (((int)S.rmax[r] - (int)S.rmin[r]) >> 1) + 1 : 0;
    const int end = 2 * (int)S.roff[r] + ns_r;
    const int rr = r - lane;
    const int start = rr >= 0 ? 2 * (int)S.roff[rr] : 0;
    const unsigned long long fits = __ballot(rr >= 0 && end - start <= CN_RING);
    const int count = __popcll(fits);                      // a prefix of the lanes (start decreases with the lane); >= 1 (a row has <= 182 cells)
    const int base = 2 * (int)S.roff[r - count + 1];
    if (lane < count) S.woff[rr & 63] = (uint16_t)(start - base);
    const int words = (end - base + 1) >> 1;               // <= CN_RING / 2
    const uint32_t* g32 = (const uint32_t*)grow + (base >> 1);
    constexpr int NW = CN_RING / 2 / 64;
    uint32_t v[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) v[j] = lane + 64 * j < words ? __hip_atomic_load(g32 + lane + 64 * j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
    for (int j = 0; j < NW; ++j)
        if (lane + 64 * j < words) ((uint32_t*)S.ring)[lane + 64 * j] = v[j];
    return r - count + 1;
}

// ASM = false: mecat2cns (jobs = mhip_aln_job: one start point, both directions from it, the strand on the x sequence).
// ASM = true: the extension of mecat2canu's mecat2asmpw / mecat2trimpw (mecat2canu/src/mecat2asmpw/mecat2asmpw.c:723-841), which is the
// code dw.cpp was derived from — same blocks, same tail rule, same failure rules — with jobs = mhip_asm_job: each direction has its
// own start point and sizes (the left extension starts on the LAST base of the seed 13-mer, the right one on its first: both contain
// the seed), the x sequence is the subject read of the indexed block (always forward), the strand applies to the y sequence (the
// mapped read), and the band is band_frac * block (0.10: `ErrorRate * s_k`, :749) where mecat2cns has 0.3.
template <bool ASM>
__global__ __launch_bounds__(CN_BLOCK, 6) void cns_extend(const uint32_t* __restrict__ rpac, const mhip_offset_t* __restrict__ roffs,
                                                       const uint32_t* __restrict__ qpac, const mhip_offset_t* __restrict__ qoffs,
                                                       const void* __restrict__ jobs_v, int n, double error_rate, double band_frac, int dir_cols_cap,
                                                       uint32_t* __restrict__ ops, CnsDir* __restrict__ dres, uint16_t* __restrict__ gscratch,
                                                       unsigned int* __restrict__ cursor, int* __restrict__ err_flag,
                                                       const uint32_t* __restrict__ rnpac, const uint32_t* __restrict__ qnpac,
                                                       const unsigned int* __restrict__ ulist /*NULL: every unit; else [0] = how many, then the units*/) {
    __shared__ CnsLds lds[CN_WAVES];
    CnsLds& S = lds[threadIdx.x >> 6];
    const int lane = lane_id();
    // mecat2asmpw / mecat2trimpw only: the planes of the bases that are not A, C, G, T (mhip_volume_set_nplane; NULL without such bases), staged
    // beside the blocks' 2-bit words in the part of V[] these tools never reach (their max_d is 120 of CN_MAX_D = 480: rows and path use the
    // first 496 bytes of the union)
    uint32_t* const Qn = (uint32_t*)&S.V[512];
    uint32_t* const Tn = Qn + CN_SEQ_WORDS;
    static_assert(1024 + 2 * CN_SEQ_WORDS * 4 <= CN_VLEN * 2, "the N planes fit behind the rows of an ASM block");
    uint16_t* grow = gscratch + (size_t)(blockIdx.x * CN_WAVES + (threadIdx.x >> 6)) * CN_GROW;
    const size_t dir_words = ((size_t)dir_cols_cap + 15) / 16;
    while (true) {
        unsigned int unit = 0;
        if (lane == 0) unit = atomicAdd(cursor, 1u);
        unit = __shfl(unit, 0);
        if (unit >= (ulist ? ulist[0] : 2u * (unsigned)n)) break;
        if (ulist) unit = ulist[1u + unit];
        const int right = unit & 1;
        SeqView q, t;
        q.pac = qpac; t.pac = rpac;
        int query_size, target_size;
        if (!ASM) {
            const mhip_aln_job jb = ((const mhip_aln_job*)jobs_v)[unit >> 1];
            const int qsize = qoffs[jb.qid_local].size, tsize = roffs[jb.sid_local].size;
            q.off = qoffs[jb.qid_local].offset; q.comp = jb.chain;
            t.off = roffs[jb.sid_local].offset; t.comp = 0;
            const int qs0 = right ? jb.qstart : jb.qstart - 1, step = right ? 1 : -1;
            if (jb.chain) { q.A = qsize - 1 - qs0; q.B = -step; } else { q.A = qs0; q.B = step; }
            t.A = right ? jb.sstart : jb.sstart - 1; t.B = step;
            query_size = right ? qsize - jb.qstart : jb.qstart;
            target_size = right ? tsize - jb.sstart : jb.sstart;
        } else {
            const mhip_asm_job jb = ((const mhip_asm_job*)jobs_v)[unit >> 1];
            const int tsize = roffs[jb.yid].size, step = right ? 1 : -1;
            q.off = qoffs[jb.xid].offset; q.comp = 0;
            t.off = roffs[jb.yid].offset; t.comp = jb.chain;
            q.A = right ? jb.rx : jb.lx; q.B = step;
            const int ys0 = right ? jb.ry : jb.ly;            // position on the mapped strand
            if (jb.chain) { t.A = tsize - 1 - ys0; t.B = -step; } else { t.A = ys0; t.B = step; }
            query_size = right ? jb.rnx : jb.lnx;
            target_size = right ? jb.rny : jb.lny;
        }
        uint32_t* uops = ops + (size_t)unit * dir_words;

        int extend1 = 0, extend2 = 0, cols = 0, n_ins = 0, n_del = 0;
        int extend_size = min(query_size, target_size);
        bool more = true;
        while (more) {      // dw_in_one_direction, dw.cpp:319-375
            int seg;
            if (extend_size > CN_SEG + 100) seg = CN_SEG;
            else { seg = extend_size; more = false; }
            if (seg <= 0) break;                         // Align "succeeds" on an empty block, then i == extend_size ends it (:356)
            const int band_tol = (int)(band_frac * seg);
            const int max_d = (int)(2.0 * error_rate * (seg + seg));
            const int koff = max_d, band_size = band_tol * 2;
            __builtin_amdgcn_wave_barrier();
            bool has_n = false;                          // (wave-uniform) the staged range of either sequence holds a base that is not A, C, G, T
            for (int w = lane; w < CN_SEQ_WORDS; w += 64) {
                const bool in = w > 0 && (w - 1) * 16 < seg + 32;
                S.Qp[w] = in ? view_word(q, extend1 + (w - 1) * 16) : 0u;
                S.Tp[w] = in ? view_word(t, extend2 + (w - 1) * 16) : 0u;
                if (ASM && (qnpac || rnpac)) {
                    SeqView qn = q, tn = t;
                    qn.pac = qnpac; qn.comp = 0; tn.pac = rnpac; tn.comp = 0;
                    const uint32_t a = (in && qnpac) ? view_word(qn, extend1 + (w - 1) * 16) : 0u;
                    const uint32_t b = (in && rnpac) ? view_word(tn, extend2 + (w - 1) * 16) : 0u;
                    Qn[w] = a; Tn[w] = b;
                    if (q.comp) S.Qp[w] = unflip_symbols(S.Qp[w], a);
                    if (t.comp) S.Tp[w] = unflip_symbols(S.Tp[w], b);
                    has_n |= (a | b) != 0u;      // (a lane may stage more than one word when the staging size grows)
                }
            }
            if (ASM) has_n = __ballot(has_n) != 0ull;
            for (int i = lane; i < 2 * max_d + 4 && i < CN_VLEN; i += 64) S.V[i] = 0;     // :329-330
            __builtin_amdgcn_wave_barrier();

            // ---- Align, forward rows (:172-210)
            int best_m = -1, min_k = 0, max_k = 0;
            int end_d = -1, end_k = 0, end_x = 0;
            int cum = 0;                                 // cells of the rows written so far (every row padded to an even length)
            for (int d = 0; d < max_d; ++d) {
                if (max_k - min_k > band_size) break;
                const int nslot = max_k >= min_k ? ((max_k - min_k) >> 1) + 1 : 0;
                if (lane == 0) { S.rmin[d] = (int16_t)min_k; S.rmax[d] = (int16_t)max_k; S.roff[d] = (uint16_t)(cum >> 1); }
                int mmax = -1, hkey = 0x7fffffff;
                constexpr int MAXJ = (CN_ROW_W + 63) / 64;
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
                    int x = (k == min_k || (k != max_k && vl < vr)) ? vr : vl + 1;       // :176-179
                    x = act ? x : seg;
                    int y = act ? x - k : 0;
                    bool again;
                    do {
                        const int lim = min(seg - x, seg - y);
                        // (such a base equals only itself, `align` compares characters: mecat2asmpw.c:316-335 feed it the reads as they are)
                        const int m = min((ASM && has_n) ? match16n(S.Qp, Qn, x, S.Tp, Tn, y) : match16(S.Qp, x, S.Tp, y), lim);
                        const int nn = min(m, 16);
                        x += nn; y += nn;
                        again = m > 16;
                    } while (__ballot(again));
                    us[j] = act ? x + y : -0x40000000;
                    if (act) {
                        grow[cum + tt] = (uint16_t)x;
                        mmax = max(mmax, x + y);
                        if (x >= seg || y >= seg) hkey = min(hkey, (kk << 10) | x);           // lowest diagonal first (:198-199)
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
                best_m = max(best_m, wave_max(mmax));
                if (__ballot(hkey != 0x7fffffff)) {      // some diagonal reached an end: the lowest one ends the block
                    hkey = wave_min(hkey);
                    end_d = d; end_k = (hkey >> 10) - koff; end_x = hkey & 1023;
                    break;
                }
                // band (:202-209): first / last diagonal within band_tol of the best; one ballot per 64 diagonals, bit scans on
                // the scalar unit
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
            if (end_d < 0) break;                        // no end reached: Align returns 0

            // ---- the path, end to start (:222-240): one scalar walk, every lane the same.  Row cd needs its two neighbours in
            // row cd - 1; the rows come back from the global scratch a window at a time.
            __threadfence();
            __builtin_amdgcn_wave_barrier();
            int rstar = -1, x2s = 0, ks = 0;             // the last row (highest d) whose snake has >= 4 matches (:336-343)
            {
                int ck = end_k, x2 = end_x, w_lo = end_d;        // rows [w_lo, ...] are in the window
                for (int cd = end_d; cd >= 0; --cd) {
                    int x1 = 0, pre = ck, px2 = 0;
                    if (cd > 0) {
                        if (cd - 1 < w_lo) {
                            __builtin_amdgcn_wave_barrier();
                            w_lo = cns_load_window(S, grow, cd - 1, lane);
                            __builtin_amdgcn_wave_barrier();
                        }
                        const int cmin = S.rmin[cd], cmax = S.rmax[cd], pmin = S.rmin[cd - 1], pmax = S.rmax[cd - 1];
                        const int kl = ck - 1, kr = ck + 1;
                        const int vl = (kl >= pmin && kl <= pmax) ? cns_cell(S, cd - 1, kl) : 0;
                        const int vr = (kr >= pmin && kr <= pmax) ? cns_cell(S, cd - 1, kr) : 0;
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
            const int ncols = carry, end_y = end_x - end_k;
            int kept_cols, kept_q, kept_t;
            if (more) {
                if (rstar < 0) break;
                const int lens = (int)(S.tlen[rstar] & 0x7FFF);
                kept_cols = (int)S.ring[rstar] + lens - 4;
                kept_q = x2s - 4;
                kept_t = x2s - ks - 4;
                if (kept_q == 0) break;                  // "i == ALN_SIZE" (:350)
            } else {
                kept_cols = ncols; kept_q = end_x; kept_t = end_y;
                if (end_x == 0) break;                   // "i == extend_size" (:356)
            }
            if (cols + kept_cols > dir_cols_cap) { if (lane == 0) atomicExch(err_flag, 1); break; }
            // ---- emit: 0 = both bases (the buffer is zero-filled), 1 = target base only, 2 = query base only
            for (int r0 = 1; r0 <= end_d; r0 += 64) {
                const int r = r0 + lane;
                const bool in = r <= end_d;
                const int c = in ? (int)S.ring[r] - 1 : 0x7fffffff;          // column of the row's indel
                const bool put = in && c < kept_cols;
                const int op = put ? ((S.tlen[r] & 0x8000) ? 2 : 1) : 0;
                if (put) {
                    const int gc = cols + c;
                    atomicOr(&uops[gc >> 4], (uint32_t)op << ((gc & 15) << 1));
                }
                n_ins += __popcll(__ballot(op == 1));
                n_del += __popcll(__ballot(op == 2));
            }
            cols += kept_cols;
            extend1 += kept_q;
            extend2 += kept_t;
            extend_size = min(query_size - extend1, target_size - extend2);
        }
        if (lane == 0) { CnsDir D = {cols, extend1, extend2, n_ins, n_del, 0}; dres[unit] = D; }
    }
}

int cns_error_word(mhip_ctx* c, int** d_err) {
    unsigned int* d_cur;
    if (c->scratch("cn_cursor", 64, (void**)&d_cur)) return -1;
    *d_err = (int*)(d_cur + 8);
    return 0;
}

int cns_extend_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const CnsExtendJobs& jobs, int dir_cols_cap, uint32_t* ops,
                      CnsDir* dres) {
    const int max_waves = c->num_cus * 24;                          // 6.3 KB of LDS per wave, <= 80 VGPRs
    const int grid = std::min(max_waves / CN_WAVES, (2 * jobs.n + CN_WAVES - 1) / CN_WAVES);
    uint16_t* d_g;
    unsigned int* d_cur;
    if (c->scratch("cn_rows", sizeof(uint16_t) * CN_GROW * (size_t)max_waves, (void**)&d_g)) return -1;
    if (c->scratch("cn_cursor", 64, (void**)&d_cur)) return -1;
    HIPCHK(hipMemsetAsync(d_cur, 0, sizeof(unsigned int), c->stream));
    const auto launch = [&](const char* name, auto kernel, const uint32_t* rnpac, const uint32_t* qnpac) {
        LAUNCH(c, name, kernel, grid, CN_BLOCK, 0, (const uint32_t*)ref->d_pac, (const mhip_offset_t*)ref->d_offs, (const uint32_t*)reads->d_pac,
               (const mhip_offset_t*)reads->d_offs, jobs.d_jobs, jobs.n, jobs.error_rate, jobs.band_frac, dir_cols_cap, ops, dres, d_g, d_cur,
               (int*)(d_cur + 8), rnpac, qnpac, jobs.ulist);
    };
    if (jobs.asm_rules) launch("asm_extend", cns_extend<true>, (const uint32_t*)ref->d_npac, (const uint32_t*)reads->d_npac);
    else launch("cns_extend", cns_extend<false>, (const uint32_t*)nullptr, (const uint32_t*)nullptr);
    return 0;
}
