// xd_block_ring.h — the RING block of the X-drop aligner, the production formulation: a row's scores in an LDS ring of XW_RING cells,
// 4-bit script cells, a traceback that takes whole diagonal runs per turn.  The row formulation is the one at the head of xalign.hip,
// organised around what the counters said bounds it (profiles/r04a_config5_cell_*: both issue ports at ~40 %, 41 % of the wave time
// waiting on LDS round trips, three stores per row and 907 GB of scratch traffic per 0.75 s launch):
//   * the gap tail behind the window (:139-147) is not a second phase: the lanes behind the window run the same cell code with
//     (H', F') = (MIN, MIN) and no diagonal, their row-gap value is exactly the tail's e_end - l, and "kept" is the tail's own
//     condition (still within X of the best, b < N) — so a row is its passes and a few scalar instructions;
//   * every lane stores its (H, F) and its script cell, no predicated stores: slots of cells outside the next window are never read
//     (the ring holds 128 cells, a row at most 126); the closing (MIN, MIN) cell is one uniform store after the passes;
//   * a row's first column lives in LDS (rs[]): one store per group of rows is all that leaves the CU — the scratch traffic was what
//     capped the kernel (waves 16 -> 28: flat);
//   * the score of a dropped cell's row gap (H of the nearest kept cell to the left - 1) is a scalar for every lane behind the last
//     or in front of the first kept cell; only a row with a hole between kept cells takes the per-lane look-up;
//   * the query bases of 64 rows sit in a register (one v_readlane per row instead of an LDS round trip).
// Script cells are 4 bits (one byte per cell before: 64 bytes per row written and read back were 400 GB per launch on a
// config-5 grid cell against 1.8 GB of algorithmic bytes):
//   bits 0-1  the cell's own op: 0 = substitution over a mismatch, 1 = substitution over a match, 2 = GAP_IN_A, 3 = GAP_IN_B
//   bit 2     EXT_A (the column gap into this cell extends), bit 3 EXT_B (the row gap extends)          (xdrop_gapalign.h:13-34)
// A lane keeps the nibbles of EIGHT consecutive rows in a register (row a in bits 4 (a & 7) ..) and stores the register once per
// group of eight rows: group g of a wave's scratch = 64 dwords, lane l's dword = the cells rs[a] + l of rows 8 g .. 8 g + 7 — one
// coalesced 256-byte store per eight rows instead of a 64-byte store per row.  Cells 64.. of the rows that have them (one row in ten)
// go the same way into a second array of groups behind the first; a bit per group says whether it was written.
// A block whose window outgrows the ring ends with overflow = 2: the caller redoes it with xdrop_block_wide.  Included by xalign.hip and, with
// a view and a column sink of its own (xd_defs.h: XNoSink), by ref_xextend.hip.
#pragma once
#include <type_traits>

#include "xd_defs.h"

#define XR_GROUPS ((X_MAXN + 2 + 7) / 8 + 2)                 // groups of eight rows; two spare groups, because the traceback's first window
                                                             // loads groups (wlo >> 3) + 2 and + 3 with wlo up to (X_MAXN & ~15) - 16
#define XR_STATE_BYTES ((size_t)XR_GROUPS * 256 * 2)        // first chunks, second chunks
#define XN_GA 2
#define XN_GB 3
#define XN_EXT_A 4
#define XN_EXT_B 8
struct XrLds {
    int2 HF[XW_RING];                    // (H, F) of cell b at b mod XW_RING
    uint8_t Tb[X_MAXN + 72 + 64];        // Tb[b] = target base b - 1 (idle and tail lanes read up to 128 cells behind the window)
    uint16_t rs[X_MAXN + 4];             // first column of every row's script cells
    uint32_t win[2][4][64];              // traceback window: [chunk][group & 3][lane], 32 rows
    uint32_t two[(XR_GROUPS + 31) / 32 + 1];   // groups that wrote a second chunk (one spare word: issue_groups reads words (g0 >> 5) and + 1)
};
static_assert((((X_MAXN & ~15) - 16) >> 3) + 3 < XR_GROUPS, "the traceback's first window stays inside the wave's group arrays");

template <class View = XView, class Sink = XNoSink>
__device__ void xdrop_block_ring(XrLds& S, const View& q, int qidx, int M, const View& t, int tidx, int N, uint8_t* __restrict__ st, XBlockOut& o,
                                 const Sink& sink = Sink()) {
    xblock_clear(o);
    if (M <= 0 || N <= 0) return;
    const int lane = lane_id();
    const int X = 30;
#ifdef MECAT_XD_STATS
    unsigned long long tk0 = __builtin_amdgcn_s_memtime();
#endif
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < N; i += 64) S.Tb[i + 1] = (uint8_t)xv_at(t, tidx + i);
    const int n_init = min(N, X);
    uint32_t* __restrict__ st32 = (uint32_t*)st;                    // first chunks: group g at dwords 64 g ..
    uint32_t* __restrict__ st32b = st32 + (size_t)XR_GROUPS * 64;   // second chunks
    if (lane <= n_init) S.HF[lane] = make_int2(-lane, -lane - 1);
    if (lane < (int)(sizeof(S.two) / sizeof(S.two[0]))) S.two[lane] = 0;
    if (lane == 0) S.rs[0] = 0;
    // row 0 (xdrop_gapalign.cpp:45-57): cells 1 .. n_init are GAP_IN_A
    uint32_t acc = (lane >= 1 && lane <= n_init) ? (uint32_t)XN_GA : 0u, acc2 = 0u;
    bool g2 = false;                                     // a row of the current group wrote second-chunk cells
    auto flush = [&](const int g) __attribute__((always_inline)) {
        st32[g * 64 + lane] = acc;
        acc = 0u;
        if (g2) {
            st32b[g * 64 + lane] = acc2;
            acc2 = 0u;
            S.two[g >> 5] |= 1u << (g & 31);              // (every lane, one address)
            g2 = false;
        }
    };
    int b_size = n_init + 1, best = 0, first_b = 0, ae = 0, be = 0;
    int qreg = 0, cellacc = 0;
    const int wmax = N <= X ? -1 : 64;                   // N <= X: row 0 ran off the end of the target (b_size = N + 1), every row through the general code
    __builtin_amdgcn_wave_barrier();
    XD_TICK(tk_stage);
    // One flat loop with one exit: the compiler lays out a loop nest with early exits as a state machine of flag registers and
    // re-tested branches — 30 scalar instructions per row of pure control flow in the round-4 kernel, and the scalar side is what
    // bounds the row (moving five vector instructions of the common row to nine scalar ones cost 10 %).  A row that ends the block
    // (no kept cell, or a window the ring cannot hold) ends the loop through its bound.
    int status = 0;                                      // 1: no kept cell in the row (the block's last), 2: the window outgrew the ring
    int Mlim = M;
    // the query bases of 64 rows in a register, row a in lane a & 63: one v_readlane per row (idle lanes load a valid base: no divergent branch)
    qreg = xv_at(q, qidx + min(max(lane - 1, 0), M - 1));
    asm volatile("v_mov_b32 %0, %0" : "+v"(qreg));      // the load is waited for here, not at the row loop's first v_readlane (vmcnt also counts the groups' stores)
    XD_COUNT(n_qfill);
    int a = 1;
    for (; a <= Mlim; ++a) {
        if ((a & 7) == 0) {
            flush((a >> 3) - 1);
            if ((a & 63) == 0) {
                qreg = xv_at(q, qidx + min(a + lane - 1, M - 1));
                asm volatile("v_mov_b32 %0, %0" : "+v"(qreg));
                XD_COUNT(n_qfill);
            }
        }
        const int sh = (a & 7) << 2;
        const int AC = __builtin_amdgcn_readlane(qreg, a & 63);
        const int f0 = first_b, n0 = b_size;
        S.rs[a] = (uint16_t)f0;                                          // the row's first column (every lane, one address)
        // The common row — one pass, kept cells without a hole between them, gap tail inside the pass — with nothing but what it needs:
        // no carries, no selects for the cases it excludes (checked on the kept mask before anything is stored; a row that fails
        // the check is redone by the general code below).  Masks are compared as masks (s_bfm), "none" is s_ff1's own -1, every lane behind
        // or in front of the kept cells stores (MIN, MIN) — the closing cell is one of them, the others are never read — and the DP cells
        // are counted per lane.
        bool done = false;
        if (__builtin_expect(n0 - f0 <= wmax, 1)) {                     // (wmax = 64; -1 in a special block)
            const int b = f0 + lane;
            const bool in0 = b < n0;
            const bool live = b < N;                                     // (n0 <= N outside the special blocks)
            int2 hf = S.HF[b & (XW_RING - 1)];
            const int tb = S.Tb[b];
            const int Hp = in0 ? hf.x : X_MIN_SCORE, Fp = in0 ? hf.y : X_MIN_SCORE;
            const bool mt = AC == tb;
            const int left = xw_shr1(Hp, 0);
            const int diag = (in0 && lane != 0) ? left + (mt ? 1 : -1) : X_MIN_SCORE;
            const int Mv = max(diag, Fp);
            const int incl = xw_scan_max(Mv + b);
            const int Ec = xw_shr1(incl, XW_NEG) - b;
            const int Hc = max(Mv, Ec);
            const unsigned long long livem = __builtin_amdgcn_ballot_w64(live);
            const unsigned long long exm = __builtin_amdgcn_ballot_w64(Hc > best) & livem;
            int j1;                                                       // first cell above the best so far; -1 (as unsigned: above every lane) if none
            asm("s_ff1_i32_b64 %0, %1" : "=s"(j1) : "s"(exm));
            const int thr = best - X + ((unsigned)lane > (unsigned)j1 ? 1 : 0);
            const bool ge = Hc >= thr;
            const unsigned long long km = __builtin_amdgcn_ballot_w64(ge) & livem;
            int fkl;
            asm("s_ff1_i32_b64 %0, %1" : "=s"(fkl) : "s"(km));
            const int nk = __builtin_popcountll(km);
            unsigned long long want;                                      // nk ones from bit fkl on (0 for nk = 64: such a row fails the test)
            asm("s_bfm_b64 %0, %1, %2" : "=s"(want) : "s"(nk), "s"(fkl));
            const int lk1 = fkl + nk;                                     // one behind the last kept lane; no kept cell: -1, as unsigned above 63
            // kept cells are one run that ends in front of lane 63 (a kept lane 63 may have a gap tail behind it: general code)
            int runend;                                                   // lk1 if the kept cells are one run, else 64 (compare + select: the compiler's version is seven instructions)
            asm("s_cmp_eq_u64 %1, %2\n\ts_cselect_b32 %0, %3, 64" : "=s"(runend) : "s"(km), "s"(want), "s"(lk1) : "scc");
            if (__builtin_expect((unsigned)runend < 64u, 1)) {
                const bool kept = live && ge;
                cellacc += in0 ? 1 : 0;
                const int Hlk = __builtin_amdgcn_readlane(Hc, lk1 - 1);
                const int et = lane >= lk1 ? Hlk - 1 : X_MIN_SCORE;
                int nib = (mt && in0) ? 1 : 0;
                nib = diag < Fp ? XN_GB : nib;
                nib = Mv < (kept ? Ec : et) ? XN_GA : nib;
                const bool xa = kept && Fp >= Hc, xb = kept && in0 && Ec >= Hc;
                nib |= (xa ? XN_EXT_A : 0) | (xb ? XN_EXT_B : 0);
                acc |= (uint32_t)nib << sh;
                S.HF[b & (XW_RING - 1)] = make_int2(kept ? Hc : X_MIN_SCORE, kept ? Hc - 1 : X_MIN_SCORE);
                // a new best (all cells above the old one hold old + 1) moves (ae, be) to the first of them; the window of the next row:
                // from the first kept cell to one behind the last, where lane lk1 wrote the closing (MIN, MIN) cell unless the block ends
                // there.  Written out: the compiler tests each condition twice over (compare, select a mask, compare the mask).
                const int nbe = f0 + j1;
                asm("s_cmp_lg_u64 %[ex], 0\n\ts_cselect_b32 %[ae], %[a], %[ae]\n\ts_cselect_b32 %[be], %[nbe], %[be]\n\ts_addc_u32 %[best], %[best], 0"
                    : [ae] "+s"(ae), [be] "+s"(be), [best] "+s"(best) : [ex] "s"(exm), [a] "s"(a), [nbe] "s"(nbe) : "scc");
                first_b = f0 + fkl;
                asm("s_add_i32 %[bs], %[f0], %[lk1]\n\ts_cmp_lt_i32 %[bs], %[N]\n\ts_addc_u32 %[bs], %[bs], 0" : [bs] "=&s"(b_size) : [f0] "s"(f0), [lk1] "s"(lk1), [N] "s"(N) : "scc");
                done = true;
            }
        }
        if (!done) {
            const int nlim = max(n0, N);                 // cells that may be kept: the window, and behind it the gap tail while b < N
            o.cells += n0 - f0;
            int bb = best, rowarg = -1, fk = -1, lk = -1, lkH = 0;
            int runP = XW_NEG, prevHp = 0, et_carry = X_MIN_SCORE;
            auto pass = [&](auto first_tag, const int c0) __attribute__((always_inline)) {
                constexpr bool FIRST = decltype(first_tag)::value;
                const int b = c0 + lane;
                const bool in0 = b < n0;
                const bool live = b < nlim;
                int2 hf = S.HF[b & (XW_RING - 1)];
                const int tb = S.Tb[b];
                const int Hp = in0 ? hf.x : X_MIN_SCORE, Fp = in0 ? hf.y : X_MIN_SCORE;
                const bool mt = AC == tb;
                const int left = xw_shr1(Hp, FIRST ? 0 : prevHp);
                const bool dok = FIRST ? (in0 && lane != 0) : in0;            // no diagonal into the row's first cell, none into the gap tail
                const int diag = dok ? left + (mt ? 1 : -1) : X_MIN_SCORE;
                const int Mv = max(diag, Fp);
                const int incl = xw_scan_max(Mv + b);                         // (lanes behind the window hold MIN + b: below every real cell)
                int pex = xw_shr1(incl, XW_NEG);
                if (!FIRST) pex = max(pex, runP);
                const int Ec = pex - b;                                       // (the row's first cell: NEG - b, below MIN like the reference's MIN)
                const int Hc = max(Mv, Ec);
                const unsigned long long livem = __builtin_amdgcn_ballot_w64(live);
                const unsigned long long in0m = __builtin_amdgcn_ballot_w64(in0);
                // a row's scores exceed the best of the rows before by at most the match reward: all cells above bb hold bb + 1
                const unsigned long long exm = __builtin_amdgcn_ballot_w64(Hc > bb) & livem;
                const int j1 = exm ? __ffsll((long long)exm) - 1 : 64;
                const int thr = bb - X + (lane > j1 ? 1 : 0);
                const bool ge = Hc >= thr;
                const unsigned long long km = __builtin_amdgcn_ballot_w64(ge) & livem;
                const bool kept = live && ge;
                const int fkl = km ? __ffsll((long long)km) - 1 : 64;
                const int lkl = km ? 63 - __clzll((long long)km) : 64;       // 64: no kept cell in this pass
                const int Hlk = __builtin_amdgcn_readlane(Hc, lkl & 63);
                // the row gap a dropped cell compares with: H of the nearest kept cell to the left - 1 (MIN if none)
                int et;
                const unsigned long long holes = km ? (in0m & ~km & ((1ull << (lkl & 63)) - 1ull) & ~((2ull << (fkl & 63)) - 1ull)) : 0ull;
                if (__builtin_expect(holes == 0ull, 1)) et = lane > lkl ? Hlk - 1 : et_carry;
                else {
                    const unsigned long long lower = km & ((1ull << lane) - 1ull);
                    const int jsrc = lower ? 63 - __clzll((long long)lower) : 0;
                    const int Hj = __shfl(Hc, jsrc);
                    et = lower ? Hj - 1 : et_carry;
                }
                int nib = (mt && in0) ? 1 : 0;
                nib = diag < Fp ? XN_GB : nib;
                nib = Mv < (kept ? Ec : et) ? XN_GA : nib;
                const bool xa = kept && Fp >= Hc, xb = kept && in0 && Ec >= Hc;
                nib |= (xa ? XN_EXT_A : 0) | (xb ? XN_EXT_B : 0);
                S.HF[b & (XW_RING - 1)] = make_int2(kept ? Hc : X_MIN_SCORE, kept ? Hc - 1 : Fp);
                if (FIRST) acc |= (uint32_t)nib << sh;
                else { acc2 |= (uint32_t)nib << sh; g2 = true; }
                // carries
                if (exm) { if (rowarg < 0) rowarg = c0 + j1; bb = bb + 1; }
                if (km) {
                    if (fk < 0) fk = c0 + fkl;
                    lk = c0 + lkl;
                    lkH = Hlk;
                    et_carry = Hlk - 1;
                }
                if (FIRST) { runP = __builtin_amdgcn_readlane(incl, 63); prevHp = __builtin_amdgcn_readlane(Hp, 63); }
            };
            pass(std::integral_constant<bool, true>(), f0);
            // a second pass: the window is wider than 64 cells, or the gap tail runs on behind lane 63
            if (n0 - f0 > 64 || (lk == f0 + 63 && f0 + 64 < N)) pass(std::integral_constant<bool, false>(), f0 + 64);
            XD_COUNT(n_rows2);
            if (bb > best) { best = bb; ae = a; be = rowarg; }
            if (fk < 0) { first_b = n0; status = 1; Mlim = 0; }
            else {
                first_b = fk;
                b_size = lk + 1;
                if (b_size < N) { S.HF[b_size & (XW_RING - 1)] = make_int2(X_MIN_SCORE, X_MIN_SCORE); ++b_size; }      // the closing cell
                if (b_size - first_b > XW_RING - 2 || b_size - f0 > XW_ROWCELLS - 2) { status = 2; Mlim = 0; }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    const int arow = a - 1;                              // the last row that was run
    o.rows = arow;
    if (status == 2) { o.overflow = 2; return; }
    flush(arow >> 3);                                    // the rows of the last, partial group
    for (int off = 32; off; off >>= 1) cellacc += __shfl_xor(cellacc, off);
    o.cells += cellacc;
    o.ae = ae; o.be = be;
    XD_TICK(tk_rows);
    // ---- traceback (:165-210) fused with script_to_aligned_string + trim_mismatch_end.  Diagonal runs at once: lane i looks at cell
    // (a - i, b - i); once a step is a substitution the walk stays on the diagonal for as long as the cells' own op bits say so, so the
    // length of the run is one ballot + one bit scan, and the counters follow from the run's match bits (XTail::run).  A step that is
    // not a substitution (1 in 8 on ONT-style reads) is taken alone, or behind a run in the same turn (the cell the run stopped at is
    // already in a lane's hands).
    __threadfence();
    __builtin_amdgcn_wave_barrier();
    // The groups are read back through a 32-row LDS window (four group slots, group g in slot g & 3) that moves down the rows 16 at a
    // time, so the two groups it needs next are known in advance: their loads are in flight (in registers) while the walk is still
    // inside the current window.  The dwords were written by this wave, so they are read past the L1 (agent scope).
    uint32_t nxt[2], nxt2[2];
    bool nxt_two = false;
    auto issue_groups = [&](const int g0) __attribute__((always_inline)) {         // groups g0, g0 + 1
        nxt[0] = __hip_atomic_load(st32 + g0 * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nxt[1] = __hip_atomic_load(st32 + g0 * 64 + 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t tw = (uint32_t)((((unsigned long long)S.two[(g0 >> 5) + 1] << 32) | S.two[g0 >> 5]) >> (g0 & 31)) & 3u;
        nxt_two = __builtin_amdgcn_readfirstlane((int)tw) != 0;
        if (nxt_two) {
            nxt2[0] = __hip_atomic_load(st32b + g0 * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            nxt2[1] = __hip_atomic_load(st32b + g0 * 64 + 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    auto commit_groups = [&](const int g0) __attribute__((always_inline)) {
        S.win[0][g0 & 3][lane] = nxt[0];
        S.win[0][(g0 + 1) & 3][lane] = nxt[1];
        if (nxt_two) {
            S.win[1][g0 & 3][lane] = nxt2[0];
            S.win[1][(g0 + 1) & 3][lane] = nxt2[1];
        }
    };
    int a_index = ae, b_index = be;
    int st_op = 0;                                       // the op of the step before: 0 = substitution, XN_GA, XN_GB
    XTail T;
    int wlo = max((ae & ~15) - 16, 0);                   // first row in the window (a multiple of 16): rows [wlo, wlo + 32)
    issue_groups((wlo >> 3) + 2);
    commit_groups((wlo >> 3) + 2);
    issue_groups(wlo >> 3);
    commit_groups(wlo >> 3);
    if (wlo > 0) issue_groups((wlo >> 3) - 2);
    __builtin_amdgcn_wave_barrier();
    XD_COUNT(n_win);
    // One turn of the walk: the cells (a - i, b - i) of the diagonal in the lanes, the op of the step (the previous one while its extension
    // bit is set in this cell, else the cell's own), then either a step that is not a substitution, or the whole run of substitutions the
    // cells' own ops vouch for plus the gap step behind it.  Two loops share it: the first also looks for the tail's run of four matches
    // (trim_mismatch_end) and notes the column types the stitching needs (XTail); once those are known (a turn or two into the walk) the
    // second only counts columns and matches — the walk is a scalar program, and the bookkeeping of the first loop is most of its instructions.
    auto turn = [&](auto lean_tag) __attribute__((always_inline)) {
        constexpr bool LEAN = decltype(lean_tag)::value;
        if (wlo > 0 && a_index - wlo < 8) {              // (a step ends at row wlo - 1 at the lowest: inside the next window)
            __builtin_amdgcn_wave_barrier();
            commit_groups((wlo >> 3) - 2);
            wlo -= 16;
            if (wlo > 0) issue_groups((wlo >> 3) - 2);
            __builtin_amdgcn_wave_barrier();
            XD_COUNT(n_win);
        }
        XD_COUNT(n_steps);
        const int ri = a_index - lane, bi = b_index - lane;
        const bool vl = lane < 32 && ri >= max(wlo, 1) && bi >= 1;
        const int row = vl ? ri : a_index;
        const int rs = S.rs[row];
        const int ci = (vl ? bi : b_index) - rs;
        const int cc = min(max(ci, 0), XW_ROWCELLS - 1);
        // (a cell on the walk lies inside its row's window, so its chunk is in the window arrays; what an idle lane reads is not used)
        const uint32_t word = S.win[cc >> 6][(row >> 3) & 3][cc & 63];
        const int nib = (int)((word >> ((row & 7) << 2)) & 15u);
        const uint32_t vm = (uint32_t)__builtin_amdgcn_ballot_w64(vl && ci >= 0 && ci < XW_ROWCELLS);    // cells the window vouches for
        const uint32_t sm = (uint32_t)__builtin_amdgcn_ballot_w64((nib & 2) == 0) & vm;                  // ... whose own op is a substitution
        const uint32_t mm = (uint32_t)__builtin_amdgcn_ballot_w64((nib & 1) != 0);
        const int nib0 = __builtin_amdgcn_readfirstlane(nib);
        const int ext = st_op == XN_GA ? (nib0 & XN_EXT_A) : st_op == XN_GB ? (nib0 & XN_EXT_B) : 0;
        const int own = (nib0 & 2) ? (nib0 & 3) : 0;
        int op = ext ? st_op : own;
        int r = 1, cq = 1, ct = 1;                       // steps of this turn; what the (single) step takes when it is not a run
        uint32_t Mm = (uint32_t)nib0 & 1u;                 // match bits of the turn's substitution steps
        if (op != 0) { cq = op != XN_GA; ct = op != XN_GB; Mm = 0u; sink.gap(T.n, cq ? 2 : 1); }
        else if (sm & 1u) {                              // (else: a substitution at a cell of row or column 0, alone)
            r = sm == 0xffffffffu ? 32 : __builtin_ctz(~sm);
            Mm = mm & (r >= 32 ? 0xffffffffu : ((1u << r) - 1u));
        }
        if (!LEAN) {
            T.column_type(cq | (ct << 1) | ((int)(Mm & 1u) << 2));
            if (op != 0) T.m = 0;
            else T.run(r, Mm, a_index, b_index);
        }
        T.n += r;
        T.nmatch += __builtin_popcount(Mm);
        a_index -= cq ? r : 0;
        b_index -= ct ? r : 0;
        // the cell a run stopped at, when the window vouches for it, holds a gap op of its own (after a substitution the cell's own
        // op counts): that step in the same turn
        if (op == 0 && r < 32 && ((vm >> r) & 1u)) {
            op = __builtin_amdgcn_readlane(nib, r) & 3;
            const int gq = op != XN_GA, gt = op != XN_GB;
            a_index -= gq;
            b_index -= gt;
            sink.gap(T.n, gq ? 2 : 1);
            if (LEAN) ++T.n;
            else T.gap_after_run(gq, gt);
        }
        st_op = op;
    };
    while ((a_index > 0 || b_index > 0) && (!T.found || T.want_l1)) turn(std::false_type{});
    while (a_index > 0 || b_index > 0) turn(std::true_type{});
    // groups that were asked for and never needed are waited for here: left pending, their loads would put a vmcnt(0) wait — which also
    // waits for the stores of the groups before — at the head of the next block's row loop
    asm volatile("" :: "v"(nxt[0]), "v"(nxt[1]), "v"(nxt2[0]), "v"(nxt2[1]));
    T.finish(ae, be, o);
    XD_TICK(tk_trace);
}
