// dw_extend2.hip — the dw extension's main kernel: two (candidate, direction) units per wave, one per 32-lane half.
// dw_extend2<false> is mecat2pw's aligner, the first launch of align.hip's two-launch scheme; dw_extend2<true> is `cns_forward`, the
// forward rows of the mecat2cns re-aligner (cns_fwd.h).  (-DMECAT_DW_STATS: per-row debug counters, `make dwstats`.)
// What the aligner replaces in the reference, and why counts are all mecat2pw needs of a path, is told in dw_extend.hip.
//
// The adaptive band keeps ~26 diagonals alive on average (config 2: 6.0e9 rows, 1.5e11 cells), so a whole wave per
// unit leaves 60 % of the lanes idle and the kernel is VALU-issue bound.  Here each half-wave runs its own unit with its
// own block and row counter: one pass over the row code advances both halves by one d-row of their respective blocks; a
// half whose rows ended does its tail traceback, accounting and next block setup (or pulls a new unit) while the other
// half is masked off, and rejoins the row code at its row 0.  Everything that is a
// scalar in the one-unit kernel (band limits, best point, block sizes ...) is a per-half-uniform VGPR value here (the band's
// first diagonal and the two ring positions with the lane's own offset already added); what steers the row loops — rows left, slot
// counts, lane masks of a pass — lives on the scalar unit.  Per-half row maxima: four mirrored DPP steps + v_permlane16_swap;
// first / last qualifying diagonal of the band update from the two 32-bit halves of a ballot.  d-rows live in a 1024-entry
// ring per half, packed back to back with one entry between two rows that is the row record (see row_passes).  Ring positions are LDS
// addresses and a row never straddles the ring's end — the row that would, about one in 36, starts at the ring's origin instead, where
// three reserved entries link it to the row in front (ring_relocate; the two fast loops leave through their bound for it) —, so the row
// code reads and writes at the positions as they are, the right neighbour and pass 2 by the instruction's offset, where every access had
// a v_and_or_b32 to wrap a byte counter (profiles/dw_ring_linear.md).  ~35 rows stay traceable; the rare block whose tail traceback
// needs an overwritten row, or that never reached an end of either sequence, is handed over to the one-unit kernel (dw_extend), which
// keeps every row: 0.5 % of the units.
// Snake steps compare 16 bases per v_alignbit pair on blocks staged little-endian (view_word_le); one-pass (58 %) and two-pass rows
// have loop bodies of their own.  Inside a block the row code keeps positions in doubled units (2 x is its own v_alignbit shift operand),
// counts the rows of the two fast loops on the scalar unit, and takes the band update's first diagonal and slot count from the scalar
// unit as one packed word per half (profiles/dw_row_trims.md); the code around the row loops works in base units.
// A snake step makes one compare, nn == what is left of the window, and looks closer only when an active lane has it (snake_step_end);
// idle lanes are not parked, every consumer masks them (profiles/dw_snake_compare.md).
// The staged words of a workgroup's eight halves are interleaved word-major, so that a window's byte offset is its doubled position with
// the low five bits cleared (match16_le2), and the entry between two rows is kept in a register whose upper half is large and negative
// (sep_word), so that one select per pass serves the ring store and x + y (profiles/dw_staging.md).
// The scalar side of a row is kept as short as its vector side (the kernel ran at 78 % of the device's scalar issue rate,
// profiles/dw_scalar_side.md): a two-pass row takes the lane masks of both passes from one s_bfm_b64 per half (pass_bits), and the band
// update puts its 64-bit words together by moves (pair64) and takes a half's slot count from one sum.
// A one-pass row has no test for the half that fills all of its 32 lanes (10.85 % of those rows), where no idle lane stores the entry behind
// the row: every lane stores that entry one slot to its right in front of its own store, two scalar instructions and a branch per row
// for one LDS store (row_passes; profiles/dw_row_exits.md).
// The snake step takes its minimum in 16 bits (v_min_u16, which issues at the plain-add rate), pass 2 forms its y with two plain adds and
// no register for the negated diagonal, and a two-pass row requests pass 2's two entries of the row in front right behind pass 1's, so that
// their LDS round trip runs under pass 1's snake instead of behind it (profiles/dw_row_latency.md).
// 64 VGPRs, 19 KB of LDS per four waves, eight waves per SIMD (tests/test_dw_resources_cpu.py holds the compiler to it); on its common
// path a one-pass dual row is 40 VALU (118 issue cycles) + 25 SALU, a two-pass row 62 (182) + 35 (tests/test_dw_row_latency_cpu.py
// caps the cycles, counting the rare part of the snake step too: 122 / 190; the scalar instructions as listed are 31 / 47:
// tests/test_dw_row_exits_cpu.py caps the one-pass row's, tests/test_dw_row_scalar_cpu.py the two-pass row's).  About 70 % issue-bound and
// 30 % latency-bound by its time at 32, 28 and 24 waves per CU (profiles/dw_row_latency.md; earlier: profiles/r03_dw_row_breakdown.md,
// r05_dw_attempt.md).  The code between two row loops is 10 % of a wave's life (profiles/dw_block_setup.md).  What is and is not
// settled about the row loops: DESIGN.md §6.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "cns_fwd.h"
#include "dw_defs.h"
#include "dw_helpers.h"

#ifndef RCAP
#define RCAP 1024
#endif
#define SEQ_WORDS2 48          // 736 bases + one 16-base window, 16 bases per word, no pad word
// band_tol and max_d of a full block (SEG_BLK x SEG_BLK: every block but a unit's last), as the block set-up's f64 expressions give them
constexpr int FULL_BAND_TOL = (int)(0.3 * SEG_BLK), FULL_MAX_D = (int)(.3 * (SEG_BLK + SEG_BLK));
// Per-half LDS, 2.4 KB incl. the ring below (19 KB per workgroup of four waves: eight workgroups per CU).  There is no V[] array: row d
// reads the furthest x of diagonals k - 1 and k + 1 of row d - 1 straight from that row's entries in the ring, at pbase + tt and
// pbase + tt + 1 (inside the band they are entries of that row; at its two edges the entry between rows or a dropped diagonal: see
// the start point in row_passes).
// The staged words of a workgroup's eight halves are interleaved word-major (match16_le2): word w of half u = 2 wave + half at
// Qp[w][u] / Tp[w][u], 384 bytes per half as before.
struct StagedLds {
    uint32_t Qp[SEQ_WORDS2][AL_WAVES * 2];
    uint32_t Tp[SEQ_WORDS2][AL_WAVES * 2];
};
#define STAGED_T_BYTES ((int)offsetof(StagedLds, Tp))
// The ring of d-rows of a half: 16-bit rows of doubled x packed back to back (in front of row 0: -2, 0, -2, see the block set-up).
// Positions (lin, pbase, rlin) are LDS byte addresses and a row never straddles the ring's end, so every access of the row code is a
// ds_read_i16 / ds_write_b16 of the position as it is, the second pass and the right neighbour by the instruction's immediate offset:
// no address arithmetic per access (profiles/dw_ring_linear.md).  A row that would not fit in front of the end — a row of one or two
// passes stores ROW_STORE bytes from its start whatever its slots, a wider one its own extent — is relocated to the ring's origin
// instead (ring_relocate, about once in 36 rows of a half), where three entries are reserved:
//   entries 0 and 1, one 32-bit word: the link — the ring offset of the entry behind the last row in front of the relocation — in its
//     low 11 bits, above it the skew — the entries skipped by this block's relocations, for `cells`;
//   entry 2: a copy of that entry behind the last row, so that the relocated row, which starts at entry RING_ORG = 3, has "the entry
//     left of the row" where every row has it.
// The tail traceback steps from a row at entry RING_ORG (row 0 of a block starts at entry 6: never there) to the row in front of it
// through the link; rows of the lap before stay traceable while they are ROW_STORE bytes ahead of the write point.
#define RING_ORG 3
#define ROW_STORE 128u
typedef __attribute__((address_space(3))) uint16_t lds_u16_t;
typedef __attribute__((address_space(3))) int16_t lds_i16_t;
template <int OFF = 0> __device__ __forceinline__ int ring_ld(uint32_t pos) { return (int)((lds_i16_t*)(uintptr_t)pos)[OFF / 2]; }
template <int OFF = 0> __device__ __forceinline__ void ring_st(uint32_t pos, int x) { ((lds_u16_t*)(uintptr_t)pos)[OFF / 2] = (uint16_t)x; }
#define RING_LINK_BITS 11
static_assert(2 * RCAP == 1 << RING_LINK_BITS, "a ring offset is the low bits of the word at the origin");

// The entry between two rows, as the register that idle lanes select (sepv): rec = slots of the row | left cut of the row before << 8, below
// 2^15.  The low 16 bits — all that is stored in the ring and all a reader sees — are ~rec, a negative 16-bit number; the upper half makes
// the whole register about -2^29, so that an idle lane's x + y, formed from it, never reaches a band threshold or a row maximum without a
// select of its own.  One v_xor_b32 with a literal, where ~rec was one v_not_b32.
__device__ __forceinline__ int sep_word(int rec) { return rec ^ (int)0xE000FFFFu; }

// mask of the lanes where p holds, without the bool -> int -> compare round trip of __ballot
#define BALLOT(p) __builtin_amdgcn_ballot_w64(p)

// max over each 32-lane half, returned in every lane of the half: four mirrored DPP steps leave each 16-lane row with its
// maximum in every lane; v_permlane16_swap (gfx950) then exchanges rows 1 <-> 0 and 3 <-> 2 between two copies.
// Written with the DPP builtin (old = the identity of max, so the DPP combiner fuses mov_dpp + max into one v_max_i32_dpp) rather
// than as one asm block: the compiler then fills the two wait states each step needs with independent instructions of the row
// instead of s_nops (the first step is asm, three-address: its input stays live for the band update without a copy).
template <int CTRL> __device__ __forceinline__ int dpp_max_step(int v) {
    return max(v, __builtin_amdgcn_update_dpp((int)0x80000000, v, CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ int half_max(int v0) {
    int v;                               // quad_perm:[1,0,3,2], into a register of its own: the caller keeps v0 (no copy in front of the chain)
    asm("s_nop 1\n\tv_max_i32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(v) : "v"(v0));
    v = dpp_max_step<0x4E>(v);           // quad_perm:[2,3,0,1]
    v = dpp_max_step<0x141>(v);          // row_half_mirror
    v = dpp_max_step<0x140>(v);          // row_mirror: every lane of a 16-lane row holds the row's maximum
    int r = v, w = v;
    // rows 1 <-> 0 and 3 <-> 2 between the two copies (the wait states around it are not known to the compiler's hazard recogniser)
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(r), "+v"(w));
    return max(r, w);
}
__device__ __forceinline__ int half_min(int v) { return -half_max(-v); }

// n bits set from bit `off` up (s_bfm_b64; 0 <= n <= 32, off 0 or 32: a half's lane mask already in its half of the wave's mask)
template <int OFF> __device__ __forceinline__ unsigned long long bits_at(int n) {
    unsigned long long r;
    asm("s_bfm_b64 %0, %1, %2" : "=s"(r) : "s"(n), "n"(OFF));
    return r;
}

// Two 32-bit scalar values as one 64-bit value, low word first.  Written as a two-element vector, which the compiler builds by placing the
// two words in a register pair (at most two s_mov_b32); `(uint64_t)hi << 32 | lo` and its masked 64-bit forms it lowers to zero-extensions
// through a zero register and an s_or_b64.
typedef uint32_t dw_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned long long pair64(uint32_t lo, uint32_t hi) {
    const dw_u32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned long long, v);
}
__device__ __forceinline__ uint32_t word_lo(unsigned long long v) { return __builtin_bit_cast(dw_u32x2, v).x; }
__device__ __forceinline__ uint32_t word_hi(unsigned long long v) { return __builtin_bit_cast(dw_u32x2, v).y; }

// The lane masks of both passes of a two-pass row of one half: the low n bits of 64 (s_bfm_b64 takes six bits of n: 0 <= n <= 63).  The
// low word is the half's pass-1 mask, min(n, 32) bits, the high word its pass-2 mask, max(n - 32, 0) bits: no clamp, no subtraction.
__device__ __forceinline__ unsigned long long pass_bits(int n) {
    unsigned long long r;
    asm("s_bfm_b64 %0, %1, 0" : "=s"(r) : "s"(n));
    return r;
}

// the same for any wave-uniform n: min(max(n, 0), 32) bits (the clamp written out on the scalar unit: three scalar instructions where
// the compiler turns it into a vector v_med3)
template <int OFF> __device__ __forceinline__ unsigned long long clamped_bits_at(int n) {
    unsigned long long r;
    int c;
    asm("s_min_i32 %1, %2, 32\n\ts_max_i32 %1, %1, 0\n\ts_bfm_b64 %0, %1, %3" : "=s"(r), "=&s"(c) : "s"(n), "n"(OFF) : "scc");
    return r;
}

// The end of a snake step of dw_extend2 (see row_passes).  at_lim: the lanes with nn == limc, i.e. whose window (limc == 32 == nn) or block
// (limc < 32) ran out in this step; amask: the pass's active lanes.  Returns the active lanes that want another step (nn == 32).  No
// active lane in at_lim — 97 % of the passes — is one s_and_b64 and a branch.  Otherwise, once no lane goes on, the active lanes of
// at_lim are the diagonals that reached an end of the block (a lane that ended in an earlier step has limc == 0 == nn in the later ones):
// they are added to `ended`, and the row loops' count-down (rows_more >= 0 here) gets its two top bits set, which takes the row loop out
// through its bound (ROWS_ENDED; rows_more_value() gives the count back).
// One asm statement with a forward branch inside: written as an `if` in the snake loop, the rare part gives the loop a second exit or a
// block between its header and its latch, and the compiler (loop-exit unification, CFG structurisation: they run on uniform branches
// too) then carries flag registers, their moves and a second re-tested branch around every step (profiles/dw_snake_compare.md).
#define ROWS_ENDED 0xc0000000u
__device__ __forceinline__ unsigned long long snake_step_end(unsigned long long at_lim, unsigned long long amask, int nn,
                                                             unsigned long long& ended, int& rows_more) {
    unsigned long long more;
    int mark;
    asm("s_and_b64 %[more], %[at], %[am]\n\t"
        "s_cbranch_scc0 1f\n\t"
        "v_cmp_eq_u32 vcc, 32, %[nn]\n\t"
        "s_and_b64 vcc, vcc, %[more]\n\t"             // the lanes that go on; SCC: there are some
        "s_cselect_b64 %[more], 0, %[more]\n\t"       // the lanes that ended, once nobody goes on
        "s_cselect_b32 %[mark], 0, 0xc0000000\n\t"
        "s_or_b32 %[rm], %[rm], %[mark]\n\t"
        "s_or_b64 %[en], %[en], %[more]\n\t"
        "s_mov_b64 %[more], vcc\n"
        "1:"
        : [more] "=&s"(more), [mark] "=&s"(mark), [en] "+s"(ended), [rm] "+s"(rows_more)
        : [at] "s"(at_lim), [am] "s"(amask), [nn] "v"(nn)
        : "vcc", "scc");
    return more;
}
// the count-down behind a row: what it would be had snake_step_end not marked it (the caller has taken the row off: - 1)
__device__ __forceinline__ int rows_more_value(int rows_more, bool marked) {
    return marked ? (int)(((unsigned)rows_more + 1u) & ~ROWS_ENDED) - 1 : rows_more;
}

#ifndef DW2_WAVES_PER_SIMD
#define DW2_WAVES_PER_SIMD 8
#endif
// CNS = false: mecat2pw's aligner (DiffAligner::go).  CNS = true: the forward rows of mecat2cns' re-aligner (dw.cpp:146-375; cns_fwd.h) —
// the same d-rows under its block rules (square blocks of 500, or the rest when it is <= 600; max_d from the error rate; a block that
// reaches no end ends the direction: no best-point fallback; every block but the last is cut in front of its last four matches), plus
// a 16-byte record per row in the row log and a record per block that contributes columns, for cns_trace to find the paths.
#ifndef CNS_FWD_WAVES_PER_SIMD
#define CNS_FWD_WAVES_PER_SIMD 8
#endif
template <bool CNS>
__global__ __launch_bounds__(AL_BLOCK, CNS ? CNS_FWD_WAVES_PER_SIMD : DW2_WAVES_PER_SIMD) void dw_extend2(const uint32_t* __restrict__ rpac, const mhip_offset_t* __restrict__ roffs,
                                                       const uint32_t* __restrict__ qpac, const mhip_offset_t* __restrict__ qoffs,
                                                       const mhip_aln_job* __restrict__ jobs, int n, DirResult* __restrict__ dres,
                                                       DwHandover* __restrict__ hand, unsigned int* __restrict__ hand_count,
                                                       unsigned int* __restrict__ cursor, unsigned long long* __restrict__ counters,
                                                       const CnsFwdArgs ca) {
    // one object, so that the staged words sit behind the 16 KB of rings, which is 2 KB-aligned (match16_le2 ORs a window's offset into
    // the address), and the workgroup's LDS stays 19 456 bytes whatever order the compiler would give two arrays
    struct DwLds {
        uint16_t rings[AL_WAVES * 2][RCAP];
        StagedLds staged;
    };
    static_assert(offsetof(DwLds, staged) % 2048 == 0 && 32 * SEQ_WORDS2 <= 2048 && sizeof(uint32_t) * AL_WAVES * 2 == 32,
                  "a window's byte offset x2 & ~31 and the address of a half's word 0 have no bit in common");
    __shared__ __attribute__((aligned(2 * RCAP))) DwLds lds;
    const int lane = lane_id(), hh = lane >> 5, sl = lane & 31;
    const int half_u = (threadIdx.x >> 6) * 2 + hh;
    const uint32_t rbase0 = (uint32_t)(uintptr_t)(lds_u16_t*)&lds.rings[half_u][0];
    const uint32_t ubase = (uint32_t)(uintptr_t)(lds_u32_t*)&lds.staged.Qp[0][half_u];      // the half's word 0 of the query (match16_le2)
    // Ring positions are LDS addresses with the lane's own 2 sl added.  org_l: entry RING_ORG, where a relocated row starts; wrap_l: the
    // last position a row of one or two passes may start at (its passes store ROW_STORE bytes from there and the entry behind it may take
    // two more: nothing is ever stored beyond the half's 2 KB — the next half's ring or the staged words sit there).
    // wrap_l is the one value kept across the row loops: the ring's base is its address bits above the ring's size (RING_BASE, good for any
    // address inside the ring), and org_l a constant below it.
    const uint32_t wrap_l = rbase0 + (2u * RCAP - ROW_STORE - 2u) + 2u * sl;
#define RING_BASE(p) ((p) & ~(2u * RCAP - 1u))
#define org_l (wrap_l - (2u * RCAP - ROW_STORE - 2u - 2u * RING_ORG))
    // nev: what a half counts, one kind per lane of one register — lane 0 of the half the units handed over (NEV_HAND), lane 1 the rows
    // relocated to the ring's origin, lane 2 the tail-walk steps taken through a link, lane 3 the blocks, lane 4 the cells (one register
    // across the row loops where each count had its own); summed per kind at the kernel's end
    unsigned int nev = 0;
    enum { NEV_HAND = 0, NEV_RELOC = 1, NEV_LINK = 2, NEV_BLOCKS = 3, NEV_CELLS = 4 };
#ifdef MECAT_DW_STATS
    // development build only (tools/dev/dw_breakdown.sh -> profiles/rNN_dw_row_breakdown.md): where the wave's time and rows go.
    // Clocks are s_memrealtime ticks (100 MHz), summed per section over the wave's life; counts are per dual row.
    unsigned long long nrows = 0, nidle = 0, nwide = 0;
    unsigned long long tk_rows = 0, tk_setup = 0, tk_ended = 0, tk_trace = 0, tk_acct = 0, n_outer = 0, n_setup = 0, n_ended = 0, n_pass3 = 0;
    unsigned long long nh[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // unit rows by band width: <= 8, 16, 24, 32, 48, 64, 96, more
    unsigned long long q16[6] = {0, 0, 0, 0, 0, 0};           // unit rows by ceil(nslot / 16): 1, 2, 3, 4, 5-6, more
    unsigned long long snake2 = 0;                            // snake steps beyond the first (per pass)
    unsigned long long n_one = 0, n_one32 = 0;               // dual rows of at most 32 slots per half with both halves in a block; those with a half at exactly 32
    const unsigned long long tk_start = wall_clock64();
#define DWS_T(var) const unsigned long long var = wall_clock64()
#define DWS_ADD(acc, a, b) acc += (b) - (a)
#else
#define DWS_T(var)
#define DWS_ADD(acc, a, b)
#endif

    // per-half unit state (uniform inside a half)
    bool need_unit = true, exhausted = false;
    bool setup = true;          // the half is between blocks
    bool inblock = false;       // the half has a block whose rows are running or have just ended
    unsigned int unit = 0;
    SeqView q, t;
    q.pac = qpac; t.pac = rpac; q.off = 0; t.off = 0; q.A = q.B = t.A = t.B = 0; q.comp = t.comp = 0;
    int query_size = 0, target_size = 0, qidx = 0, tidx = 0;
    int Rq = 0, Rt = 0, Rm = 0, Rc = 0, Rb = 0;
    // per-half block state.  The block's two lengths and its band tolerance are kept in the row loops' doubled units (`2`, see below) and
    // halved where the code around the loops wants them: kept in both forms they would cost three registers across the row loops.
    int q_len2 = 0, t_len2 = 0, last_block = 0, band_tol2 = 0, max_d = 0;
    // band = nslot diagonals from min_k; d = rows done.  The three values every lane adds its own 2 * sl to on every row are kept with
    // it added (`_l`: per lane): the row code then uses them as they are, and the band update moves all lanes by the same amount.
    int best_m = -1, mk_l = 0, nslot = 0, d = 0;
    int sepv = sep_word(1);     // what idle lanes store behind the row: sep_word(slots of the row | left cut of the row before << 8), see row_passes
    int cut = 0;                // diagonals the last band update dropped on the left (`first`)
    // (ring positions are LDS addresses; a half that never gets a block stores like the others while the other half rows: inside its ring)
    unsigned int lin_l = org_l + 6u;     // ring position behind the last row (an address, like the next two) + 2 sl
    unsigned int pb_l = org_l;           // ring position of the previous row's entry for diagonal (this row's min_k) - 1, + 2 sl
    unsigned int rlin_l = org_l;         // ring position of the row that ran last, + 2 sl
    int dlim = 0;               // rows run while d < dlim: max_d of the block, 0 once an end was reached / without a block
    // CNS: the unit's share of the row log [logpos, logend), the record of the current block's row 0, and whether the unit met something
    // the log cannot hold: more rows than its share, or a row of more than 96 diagonals (a record holds three passes of 32; the pass count is
    // the wave's, so a fourth pass for the other half's row sends this half's unit along).  Such a unit is handed over to cns_extend, like
    // one whose tail walk left the ring or met a cut of 127 or more, or whose block records are used up
    // (tests/test_gpu_cns_forward_edges.py: rows of 96 diagonals stay, wider ones leave).
    unsigned int logpos = 0, logend = 0, blk_log0 = 0, blkpos = 0, blkend = 0;
    bool cns_bad = false;
    unsigned long long fl0 = 0, fl1 = 0, fl2 = 0;      // lanes whose diagonal came from k - 1, first / second / third pass of the row that ran last
    int last_ns = 0;                           // its slots

    while (true) {
#ifdef MECAT_DW_STATS
        n_outer += 1;
        n_setup += BALLOT(setup) ? 1u : 0u;
#endif
        DWS_T(t_a);
        if (BALLOT(setup)) {
            // ---- 1. a half without a unit pulls the next one
            if (setup && need_unit) {
                unsigned int u = 0;
                if (sl == 0) u = atomicAdd(cursor, 1u);
                u = __shfl(u, hh << 5);
                if (u >= 2u * (unsigned)n) { exhausted = true; setup = false; mk_l = 4 * sl; nslot = 0; dlim = 0; }      // never rowing
                else {
                    unit = u;
                    const mhip_aln_job jb = jobs[u >> 1];
                    const int right = u & 1;
                    const int qsize = qoffs[jb.qid_local].size, tsize = roffs[jb.sid_local].size;
                    q.off = qoffs[jb.qid_local].offset; q.comp = jb.chain;
                    t.off = roffs[jb.sid_local].offset; t.comp = 0;
                    const int qs0 = right ? jb.qstart : jb.qstart - 1, step = right ? 1 : -1;
                    if (jb.chain) { q.A = qsize - 1 - qs0; q.B = -step; } else { q.A = qs0; q.B = step; }
                    t.A = right ? jb.sstart : jb.sstart - 1; t.B = step;
                    if (right) { query_size = qsize - jb.qstart; target_size = tsize - jb.sstart; }
                    else { query_size = jb.qstart; target_size = jb.sstart; }
                    if (jb.qstart < 0 || jb.sstart < 0) { query_size = 0; target_size = 0; }      // (see dw_extend)
                    qidx = tidx = 0;
                    Rq = Rt = Rm = Rc = Rb = 0;
                    need_unit = false;
                    if (CNS) { logpos = ca.logbase[u]; logend = ca.logbase[u + 1]; blkpos = ca.blockbase[u]; blkend = ca.blockbase[u + 1]; cns_bad = false; }
                }
            }
            // ---- 2. block setup: retrieve_next_aln_block (gapalign.cpp:9-45) + staging
            if (setup) {
                const int qleft = query_size - qidx, tleft = target_size - tidx;
                int qblk, tblk, band_tol;
                if (CNS) {      // dw_in_one_direction, dw.cpp:319-332
                    const int ext = min(qleft, tleft);
                    if (ext > SEG_BLK + 100) { qblk = SEG_BLK; last_block = 0; } else { qblk = max(ext, 0); last_block = 1; }
                    tblk = qblk;
                    if (last_block) {
                        band_tol = (int)(0.3 * qblk);
                        max_d = (int)(2.0 * ca.error_rate * (qblk + qblk));
                    } else { band_tol = FULL_BAND_TOL; max_d = ca.full_max_d; }      // (of the launch: cns_forward_launch)
                    blk_log0 = logpos;
                    if (logend - logpos < (unsigned)max_d) { cns_bad = true; max_d = 0; }      // the rows of this block may not fit the unit's share of the log
                } else {
                if (qleft < SEG_BLK + 100 || tleft < SEG_BLK + 100) {
                    qblk = min(qleft, (int)(tleft + tleft * 0.2));
                    tblk = min(tleft, (int)(qleft + qleft * 0.2));
                    last_block = 1;
                    qblk = max(qblk, 0);
                    tblk = max(tblk, 0);
                    band_tol = (int)(0.3 * (qblk > tblk ? qblk : tblk));
                    max_d = (int)(.3 * (qblk + tblk));
                } else { qblk = SEG_BLK; tblk = SEG_BLK; last_block = 0; band_tol = FULL_BAND_TOL; max_d = FULL_MAX_D; }      // no f64 for a full block
                }
                // Staging: word w = logical bases 16w .. 16w+15, first base in the low bits, in the half's own column of the interleaved
                // array (a live window stays in it: its words are below SEQ_WORDS2, so the OR of match16_le2 is an add).  Only the words that hold a base of the
                // block are written (16 w < blk); the others keep what an earlier block left there, and no result depends on it:
                // a live diagonal has x <= q_len and its window is words x >> 4 and (x >> 4) + 1, so every base it sees at or beyond
                // q_len (t_len for the target) sits at window offset >= lim = min(q_len - x, t_len - y).  A first difference in
                // front of lim lies inside the valid bases of both sequences, and anything at or behind lim is clamped away by
                // min(m, min3(q_len - x, t_len - y, 16)); the end test nn == limc is decided by the same two cases.  Idle lanes keep nothing.
                // Words 32 .. are staged only when a half in set-up has a block of more than 512 bases (a last block; the test is
                // wave-uniform): a full block stages in one trip.
                static_assert((SEG_BLK + 99) * 6 / 5 <= 16 * (SEQ_WORDS2 - 1), "the longest block and one 16-base window fit the staged words");
                const int trips = BALLOT(max(qblk, tblk) > 512) ? 2 : 1;
#pragma unroll 1
                for (int w = sl, i = 0; i < trips; w += 32, ++i) {      // (blk <= 1.2 * (SEG_BLK + 99): 16 w < blk keeps w below SEQ_WORDS2)
                    lds_u32_t* const sw = (lds_u32_t*)(uintptr_t)(ubase + 32u * (unsigned)w);      // Qp[w][u]; Tp[w][u] is STAGED_T_BYTES behind it
                    if (w * 16 < qblk) sw[0] = view_word_le(q, qidx + w * 16);
                    if (w * 16 < tblk) sw[STAGED_T_BYTES / 4] = view_word_le(t, tidx + w * 16);
                }
                // The reference zero-fills V per block (:232-233); row d only reads diagonals written by row d - 1, except row 0,
                // which reads V[k_offset - 1] and V[k_offset + 1]: the two zeros in front of row 0.
                // Between two rows of the ring sits one entry of -2 or less (see the start point below); in front of row 0: -2, 0, -2 — row 0
                // reads the first two (x2 = max(-2 + 2, 0) = 0), row 1 reads the third as the entry "left of row 0".
                // They sit behind the three reserved entries at the ring's origin (ring_relocate): the word of entries 0 and 1 is cleared — no
                // bytes skipped in this block yet —, entry 2 is written by the first relocation.
                if (sl < 6) ring_st(org_l - 2u * RING_ORG, sl == 3 || sl == 5 ? -2 : 0);
                best_m = -2; mk_l = 4 * sl; nslot = 1; sepv = sep_word(1); cut = 0;
                d = 0;
                lin_l = org_l + 6u; pb_l = org_l; rlin_l = org_l;
                dlim = max_d; inblock = true;
                q_len2 = 2 * qblk; t_len2 = 2 * tblk; band_tol2 = 2 * band_tol;
                setup = false;
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (!BALLOT(!exhausted)) break;
        const int k_offset = max_d;
        // Inside a block the row code keeps positions in doubled units (`2`: x2 = 2 x, y2 = 2 y, diagonal k2 = 2 k; with them x + y of
        // the band threshold, best_m and mk_l): a position is then its own v_alignbit shift operand (match16_le2).  Ring entries are
        // x2 (at most 2 * 736 = 1472: still 16 bits, and the entries between rows stay negative); ring positions, cut, slot counts, the
        // row log and `cells` are what they were, and everything behind the end-of-block scan is in base units again.
        DWS_T(t_b);
        DWS_ADD(tk_setup, t_a, t_b);

        // ---- 3. one row per half (Align, diff_gapalign.cpp:107-219); the halves' row counters are independent.  Only the
        // running maximum of x + y is tracked here; a block that ends without reaching an end of either sequence (0.06 %
        // of blocks) needs the position of that maximum and is handed over to dw_extend, like a block whose traceback outran
        // the ring.  The inner loop runs while every half that has a block is still rowing.
        const unsigned long long inmask = BALLOT(inblock);
        // Where a block reached an end: set by the end-of-block scan below and used up in the same trip — the scan ends the block's rows
        // (dlim = 0), so its tail walk and accounting follow at once —, so nothing of it is carried across the row loops.  end_d < 0: no end.
        int end_x = 0, end_k = 0, end_d = -1, end_mk = 0;
        bool row_ok;
        unsigned long long ended = 0;        // lanes whose diagonal reached an end of its block in the row that was just run
        int NJ = 1;
        // band update (:172-179) of the row at ring position rlin; m0 / mp = x + y of the lane's diagonal in the last / previous
        // pass (NJ <= 2), otherwise recomputed from the ring
        // sa / sb: the new slot counts of the two halves for the scalar unit — with both halves in a block and NJ <= 2 straight from
        // the ballots (scalar find-first / find-last), otherwise read back from the vector state
        auto band_update = [&](const int NJ, const int m0, const int mp, auto both_tag, int& sa, int& sb) __attribute__((always_inline)) {
            constexpr bool BOTH = decltype(both_tag)::value;      // both halves are in a block: no per-half guard on the band state
            // qualifying lanes first .. last of the half.  The mask of a half that is in a block is never empty: the lane that holds
            // the row maximum qualifies, and the row maximum is the running maximum (x + y grows by at least one per row along
            // the best path, which the band never prunes).
            int first, last;
            int pk = 0;      // BOTH, NJ <= 2: (new slot count | first << 8) of the lane's half, which is the next row's separator but for sep_word's XOR
            if (NJ == 1) {
                // 32 diagonals per half: one ballot; first / last set bit of the half's 32 bits with the raw instructions
                // (v_ffbl / v_ffbh return -1 for an empty mask: a half without a block, whose values are not used)
                const unsigned long long q0 = BALLOT(m0 >= best_m - band_tol2);      // (both sides doubled: the same predicate)
                if (BOTH) {
                    // the scalar unit finds first and the new slot count of both halves anyway: it hands them to the lanes packed, one
                    // word per half in a register pair, and a lane takes its half's word with the one 64-bit shift that used to fetch
                    // the half's ballot bits (then: two find-bit instructions, an add and a subtract per row on the vector unit)
                    const unsigned int wa = (unsigned int)q0, wb = (unsigned int)(q0 >> 32);
                    const int fa = __builtin_ctz(wa), fb = __builtin_ctz(wb);
                    sa = 33 - (fa + __builtin_clz(wa));
                    sb = 33 - (fb + __builtin_clz(wb));
                    unsigned long long pkw = (unsigned int)(sa | (fa << 8)) | ((unsigned long long)(unsigned int)(sb | (fb << 8)) << 32);
                    asm("" : "+s"(pkw));
                    pk = (int)(unsigned int)(pkw >> (hh << 5));
                    first = pk >> 8;
                    last = first + (pk & 0xff) - 2;
                } else {
                    const unsigned int m32 = (unsigned int)(q0 >> (hh << 5));
                    int lz;
                    asm("v_ffbl_b32 %0, %1" : "=v"(first) : "v"(m32));
                    asm("v_ffbh_u32 %0, %1" : "=v"(lz) : "v"(m32));
                    last = 31 - lz;
                }
            } else if (NJ == 2) {
                // up to 64 diagonals per half: two ballots, the half's 2 x 32 qualification bits.  Branch-free: v_ffbl / v_ffbh return
                // -1 for an empty word, which `| 32` leaves at 0xffffffff (first: unsigned min) and `^ 31` turns into -32 (last:
                // signed max; x ^ 31 == 31 - x for x in 0..31)
                const int thr = best_m - band_tol2;
                const unsigned long long q0 = BALLOT(mp >= thr), q1 = BALLOT(m0 >= thr);
                if (BOTH) {
                    // first / last qualifying diagonal of each half on the scalar unit (its 64 bits: the half's word of both ballots),
                    // handed to the lanes as one packed value per half: two moves and a select instead of two 64-bit shifts, four
                    // find-first / find-last and their merge
                    // (the words put together from 32-bit halves, four moves: pair64.  Slots = last - first + 2 with last = 63 - clz, as one
                    // sum taken from 65, the way the one-pass row does it)
                    const unsigned long long wa = pair64(word_lo(q0), word_lo(q1)), wb = pair64(word_hi(q0), word_hi(q1));
                    const int fa = __builtin_ctzll(wa), fb = __builtin_ctzll(wb);
                    sa = 65 - (fa + __builtin_clzll(wa));
                    sb = 65 - (fb + __builtin_clzll(wb));
                    // (new slot count, first: last = first + slots - 2; kept packed: the compiler would select the four values one by one)
                    unsigned long long pkw = (unsigned int)(sa | (fa << 8)) | ((unsigned long long)(unsigned int)(sb | (fb << 8)) << 32);
                    asm("" : "+s"(pkw));
                    pk = (int)(unsigned int)(pkw >> (hh << 5));
                    first = pk >> 8;
                    last = first + (pk & 0xff) - 2;
                } else {
                    const unsigned int lo32 = (unsigned int)(q0 >> (hh << 5)), hi32 = (unsigned int)(q1 >> (hh << 5));
                    unsigned int fl, fh, ll, lh;
                    asm("v_ffbl_b32 %0, %1" : "=v"(fl) : "v"(lo32));
                    asm("v_ffbl_b32 %0, %1" : "=v"(fh) : "v"(hi32));
                    asm("v_ffbh_u32 %0, %1" : "=v"(ll) : "v"(lo32));
                    asm("v_ffbh_u32 %0, %1" : "=v"(lh) : "v"(hi32));
                    first = (int)min(fl, fh | 32u);
                    last = max((int)(ll ^ 31u), (int)((lh ^ 31u) | 32u));
                }
            } else {
                int lo = 0x7fffffff, hi = -0x7fffffff;
                for (int j = 0; j < NJ; ++j) {
                    const int tt = sl + 32 * j;
                    const bool act = inblock && tt < nslot;
                    const int k2 = mk_l + 128 * j;
                    const int u = act ? 2 * ring_ld(rlin_l + 64u * (unsigned)j) - k2 : -0x40000000;      // x2 + y2 = 2 x2 - k2
                    if (act && u >= best_m - band_tol2) { lo = min(lo, tt); hi = max(hi, tt); }
                }
                first = half_min(lo); last = half_max(hi);
            }
            if (BOTH || inblock) {
                // new band [min_k + 2 first - 1, min_k + 2 last + 1] = last - first + 2 diagonals; the previous-row entry of diagonal
                // (new min_k) - 1 sits at ring position rlin + first - 1
                // (mk_l in doubled units: + 4 first - 2.  2 first is formed once, by add — a shift left issues at half the rate —, and
                // 2 first - 2 serves both updates)
                const unsigned int first2 = twice((unsigned)first), step = first2 - 2u;
                pb_l = rlin_l + step;
                nslot = last - first + 2;
                mk_l = mk_l + (int)first2 + (int)step;
                cut = first;
                // what the idle lanes of the next row store behind it: its slot count and this cut, as a negative 16-bit number — which is
                // all the start point needs of the entry between two rows.  With both halves in a row of one or two passes that is the
                // packed word, inverted in its low 16 bits (a cut below 64).  Otherwise the cut is kept to 7 bits, saturating: the tail
                // traceback hands a block over when it meets 127.  Every writer goes through sep_word, which also gives the register the
                // upper half that idle lanes' x + y is formed from.
                if (BOTH && NJ <= 2) sepv = sep_word(pk);
                else {
                    int c7;
                    asm("v_min_u16 %0, 0x7f, %1" : "=v"(c7) : "v"(first));
                    sepv = sep_word(nslot | (c7 << 8));
                }
            }
            if (!(BOTH && NJ <= 2)) { sa = __builtin_amdgcn_readlane(nslot, 0); sb = __builtin_amdgcn_readlane(nslot, 32); }
        };
        int last_m0 = 0, last_mp = 0;
        unsigned int row_bytes = 0;
        // One d-row of both halves in NJ passes of 32 diagonals per half (NJ a constant for 1 and 2: the pass loop and the previous-pass
        // bookkeeping fold away).  ns_a / ns_b: the two halves' slot counts on the scalar unit.  A row is followed in the ring by one
        // negative entry (sepv), which the first idle lane of the last pass writes: every lane of a pass stores (its x, or sepv when idle) at
        // its own position — no exec juggling around the store, no store of its own for that entry (unless a half fills its last pass to the
        // last lane: FAST 1 stores the entry for that case on every row, see the store below; behind a general row it is the caller's
        // business).  What idle lanes write beyond it is overwritten by the rows that
        // follow, except for up to 64 entries behind the last row of a block with NJ <= 2: the tail traceback's window is shortened
        // by as much (rows with more passes guard their stores).  FAST 1: 1 <= slots <= 32 in both halves, one pass; FAST 2: 1 <= slots
        // <= 63, two passes; FAST 0: anything.  rows_more: the caller's count-down of rows, which a pass marks — and `ended` gets the
        // lanes — when a diagonal reached an end of its block (snake_step_end).
        auto row_passes = [&](const int NJ, const int ns_a, const int ns_b, int& rows_more, auto fast_tag) __attribute__((always_inline)) {
            constexpr int FAST = decltype(fast_tag)::value;

            row_bytes = twice((unsigned)nslot) + 2u;
            last_ns = nslot;
            // (-2^30: the identity of the row maximum and "no previous pass" for the band update, both below anything sep_word + y gives
            // an idle lane; the general band update's recompute from the ring keeps its own select on this value: it reads x, not m0)
            int mmax = -0x40000000, m0 = -0x40000000, mp = -0x40000000;
            // FAST 2: the lane masks of both passes.  The low ns bits of 64, one s_bfm_b64 per half (pass_bits; ns <= 63), are the half's pass-1
            // mask in the low word and its pass-2 mask in the high word; the wave's mask of a pass is the two halves' words of it side by side.
            unsigned long long two_m1 = 0, two_m2 = 0;
            if (FAST == 2) {
                const unsigned long long ma = pass_bits(ns_a), mb = pass_bits(ns_b);
                two_m1 = pair64(word_lo(ma), word_lo(mb));
                two_m2 = pair64(word_hi(ma), word_hi(mb));
            }
            int vl2 = 0, vr2 = 0;               // FAST 2: pass 2's two entries of the row in front, requested next to pass 1's
            int j = 0;
            do {                                 // at least one pass (a pass over an empty band only moves idle lanes)
                const int tt = sl + 32 * j;
                // the active lanes of this pass: the low (slots - 32 j) bits of each half, made on the scalar unit from the two
                // slot counts and used as the lane predicate as it is
                unsigned long long amask;
                if (FAST == 2) {
                    amask = j == 0 ? two_m1 : two_m2;
                } else if (FAST == 1) {
                    amask = bits_at<0>(ns_a) | bits_at<32>(ns_b);
                } else {
                    amask = clamped_bits_at<0>(ns_a - 32 * j) | clamped_bits_at<32>(ns_b - 32 * j);
                }
                const bool act = __builtin_amdgcn_inverse_ballot_w64(amask);
                const int k2 = mk_l + 128 * j;                          // (doubled: lane offset 4 sl, 128 per pass)
                const unsigned int rp = pb_l + 64u * (unsigned)j;       // idle lanes read (and ignore) whatever the ring holds there
                const int vl = (FAST == 2 && j == 1) ? vl2 : ring_ld(rp), vr = (FAST == 2 && j == 1) ? vr2 : ring_ld<2>(rp);
                // FAST 2: pass 2's reads are requested here, right behind pass 1's, where they used to follow pass 1's snake and store with
                // a whole LDS round trip in the row's serial chain and nothing to overlap it (profiles/dw_row_latency.md).  The row they
                // read is the one in front, at pb_l as before: no store of this row's pass 1 lands in it (an active lane of pass 2 reads
                // at most the entry behind that row; this row starts behind that entry, or at the ring's origin).
                // An asm statement: written as ring_ld<64>(pb_l) up here, the compiler leaves the sign extension behind the snake loop
                // (ds_read_u16 + v_bfe_i32: two more instructions per row).  It therefore does not know that the two results are in
                // flight and inserts no wait for them.  None is needed: LDS returns in order and these two stand right behind pass 1's
                // two reads (the "memory" clobber keeps them there), so the wait in front of pass 1's v_max_i16 below, which takes vr,
                // covers them — and pass 2 comes behind pass 1's snake.  tests/test_dw_row_latency_cpu.py holds the listing to it: the four
                // reads in this order, a wait between them and that v_max_i16, and no instruction in between that names vl2 or vr2.
                if (FAST == 2 && j == 0) asm volatile("ds_read_i16 %0, %2 offset:64\n\tds_read_i16 %1, %2 offset:66" : "=&v"(vl2), "=&v"(vr2) : "v"(pb_l) : "memory");
                // :138-142 `if (k == min_k || (k != max_k && V[k-1] < V[k+1])) x = V[k+1]; else x = V[k-1] + 1;` as max(vl + 1, vr), in
                // doubled units max(vl + 2, vr): inside the band the two are the same thing (vl < vr <=> vr >= vl + 1).  At k == min_k the
                // entry on the left is either the entry between two rows — ~(nslot | cut << 8) with nslot >= 1, hence <= -2: vl + 2 <= 0 <=
                // vr — or a diagonal of row d - 1 that the band update dropped while its right neighbour stayed: 2 vl - (k - 1) < best - tol
                // <= 2 vr - (k + 1) in base units, i.e. vl + 1 < vr; mirrored at k == max_k (vr is negative, or a dropped diagonal with
                // vr < vl + 1).  So the two edge tests fold into the same max — in the 16-bit forms of add and max, which issue at twice the
                // rate of the 32-bit max (the result is >= 0 and comes back zero-extended).
                int x;                           // x2 (and y, limc, nn, m0 below: y2, 2 limc, 2 nn, 2 (x + y))
                {
                    int v1;
                    asm("v_add_u16 %0, 2, %1" : "=v"(v1) : "v"(vl));
                    asm("v_max_i16 %0, %1, %2" : "=v"(x) : "v"(v1), "v"(vr));
                    if (CNS) {
                        // the step the reference's traceback will read off V (dw.cpp:176-179: from k + 1 when k == min_k, or k != max_k and
                        // V[k - 1] < V[k + 1]): with the entries the ring holds at a band's two edges (see above) that is "vl >= vr"
                        // everywhere, i.e. vl + 1 > vr (doubled: vl + 2 > vr): one 16-bit compare of what is in registers anyway (idle lanes: masked by the reader,
                        // which knows the row's slots)
                        unsigned long long fb;
                        asm("v_cmp_gt_i16_e64 %0, %1, %2" : "=s"(fb) : "v"(v1), "v"(vr));
                        // (selects of values, not `if (j == 0) fl0 = fb; else ...`: the compiler sinks the three stores of that form into ONE store
                        // through a selected address, which pins fl0 .. fl2 — and with them every read in log_row — to scratch memory)
                        fl0 = j == 0 ? fb : fl0;
                        fl1 = j == 1 ? fb : fl1;
                        fl2 = j == 2 ? fb : fl2;
                    }
                }
                // 0 <= y <= t_len and x <= q_len on every live diagonal (a diagonal at an end stops the block).
                // Idle lanes are not parked: they start from whatever max(vl + 2, vr) of the ring gives them (0 .. 65535) and snake on it.
                // All they do is load.  A window's address is (position & ~31) | ubase plus a constant of at most STAGED_T_BYTES + 32
                // (match16_le2): for a position of 0 .. 65535 and more, or a negative y, that is some 32-bit number whose low bits are
                // the half's own column — inside the workgroup's allocation it reads a ring entry or a staged word of this or another
                // half, beyond it (and wrapped around 2^32: then inside or beyond again) the read returns 0; LDS reads fault nowhere
                // and nothing is written through such an address.  Nothing
                // of theirs is kept, each consumer guarding itself: the stored value is `act ? x : sepv` (FAST 0: under tt <= nslot), m0 is
                // that value + y, about -2^29 on an idle lane (so neither the row maximum nor the band update sees them), snake_step_end masks the lanes at
                // their limit with amask — an idle lane neither asks for a further step nor ends a block —, and the CNS flag bits are
                // masked by the reader with the row's slot count.  Nothing behind the passes reads a lane's x, y, limc or nn.
                // y = x - k2.  FAST 2, pass 2 (k2 = mk_l + 128): x - mk_l, then the literal -128 — two plain adds, as asm statements: left to
                // itself the compiler keeps -mk_l in a register of its own (one v_sub_u32 per row) and a scalar register for the constant, and
                // forms y with a v_add3_u32 that takes that scalar operand (profiles/dw_row_latency.md)
                int y;
                if (FAST == 2 && j == 1) {
                    asm("v_sub_u32 %0, %1, %2" : "=v"(y) : "v"(x), "v"(mk_l));
                    asm("v_add_u32 %0, 0xffffff80, %0" : "+v"(y));
                } else {
                    y = x - k2;
                }
#ifdef MECAT_DW_STATS
                snake2 -= 1;
#endif
                unsigned long long more;
                do {
#ifdef MECAT_DW_STATS
                    snake2 += 1;
#endif
                    // what is left of the window: of the query, of the target, 16 bases
                    int limc;
                    asm("v_min3_i32 %0, %1, %2, 32" : "=v"(limc) : "v"(q_len2 - x), "v"(t_len2 - y));
                    // 0..15 equal bases (doubled: 0..30), or >= 16 (0x7ffffffe) when the whole window matches.  A lane with exactly 16
                    // bases left that all match asks for one more step, which then moves nothing.
                    const int m = match16_le2<STAGED_T_BYTES>(ubase, x, y);
                    // nn = min(m, limc) in 16 bits, which issues at the plain-add rate where v_min_i32 takes twice as long: on a live lane
                    // limc is 0 .. 32 and m 0 .. 30 or 0x7ffffffe, whose low half 0xfffe is still above any limc; the result comes back
                    // zero-extended.  (An idle lane's limc may be anything: nothing of its nn is kept.)
                    int nn;
                    asm("v_min_u16 %0, %1, %2" : "=v"(nn) : "v"(m), "v"(limc));
                    // one compare per step: nn == limc, written on the minimum's operands so that it does not wait for it, holds exactly
                    // on the lanes that go on (limc == 32) or have nothing left of the query or of the target on their diagonal
                    // (limc < 32); which of the two is looked at only when an active lane has it
                    x += nn; y += nn;
                    more = snake_step_end(BALLOT(limc <= m), amask, nn, ended, rows_more);
                } while (more);
                // one select per pass: the ring takes the low 16 bits of v, and an idle lane's m0 = sepv + y is about -2^29 (sep_word; its
                // y is within +-2^17: x from 16 bits of the ring plus its snake, k2 a diagonal of the block)
                const int v = act ? x : sepv;
                // FAST 1: the entry behind a half's row of exactly 32 slots, which no idle lane of its stores, without a test for it: every
                // lane stores sepv one slot to its right first (lane i at slot i + 1), then its own value at its own slot.  The LDS
                // instructions of a wave are performed in program order, so slots 1 .. 31 end up with what their own lanes put there, as
                // without the first store, and slot 32 holds sepv: the entry behind a 32-slot row; behind a narrower one, one more of what
                // its idle lanes leave there anyway, inside ROW_STORE.  (sepv still describes this row: the band update comes later.)
                // An asm statement: as ring_st<2> the compiler merges a lane's two stores into one ds_write_b32, in which lanes i and i + 1
                // write slot i + 1 in the same instruction and the order that lets x win is gone
                // (tests/test_gpu_dw_row_exits.py, tests/test_dw_row_exits_cpu.py).
                if (FAST == 1) asm volatile("ds_write_b16 %0, %1 offset:2" : : "v"(lin_l), "v"(sepv) : "memory");
                if (NJ <= 2 || tt <= nslot) ring_st(lin_l + 64u * (unsigned)j, v);
                mp = m0;
                m0 = v + y;                         // also read by the band update (NJ <= 2); idle lanes never qualify
                mmax = NJ == 1 ? m0 : max(mmax, m0);
            } while (++j < NJ);
            last_m0 = m0; last_mp = mp;
            rlin_l = lin_l;                      // (the caller moves lin_l behind the row and the entry behind it: lin_l += row_bytes)
            __builtin_amdgcn_wave_barrier();
            // running maximum of x + y (:160-167) = the maximum of this row: the best diagonal k* of the row before qualifies for
            // the band, so k* - 1 and k* + 1 are in this row and start at least one further along
            best_m = half_max(mmax);
        };
#ifdef MECAT_DW_STATS
        auto row_stats = [&](unsigned long long rmask, int ns_a, int ns_b, int NJ) {
            nrows += 1;
            nidle += (rmask == ~0ull) ? 0u : 1u;
            nwide += NJ > 1 ? 1u : 0u;
            n_pass3 += NJ > 2 ? 1u : 0u;
            if (rmask == ~0ull && max(ns_a, ns_b) <= 32) { n_one += 1; n_one32 += max(ns_a, ns_b) == 32 ? 1u : 0u; }
            for (int hq = 0; hq < 2; ++hq) {
                if (!((rmask >> (hq << 5)) & 1ull)) continue;      // the half is not rowing
                const int ns = hq ? ns_b : ns_a;
                nh[ns <= 8 ? 0 : ns <= 16 ? 1 : ns <= 24 ? 2 : ns <= 32 ? 3 : ns <= 48 ? 4 : ns <= 64 ? 5 : ns <= 96 ? 6 : 7] += 1;
                const int p16 = (ns + 15) >> 4;
                q16[p16 <= 4 ? p16 - 1 : p16 <= 6 ? 4 : 5] += 1;
            }
        };
#define DWS_ROW(rmask, a, b, nj) row_stats(rmask, a, b, nj)
#else
#define DWS_ROW(rmask, a, b, nj)
#endif
        // CNS: the record of the row that just ran and of the band update behind it (cns_fwd.h).  Every lane of a half stores the same 16
        // bytes at the same place: no lane predicate to set up, and the coalescer makes one write of it.
        auto log_row = [&](const int NJ, auto both_tag) __attribute__((always_inline)) {
            if constexpr (CNS) {
                constexpr bool BOTH = decltype(both_tag)::value;
                if (BOTH || inblock) {
                    // (a block's rows fit the unit's share: checked when the block is set up.  A record holds a row of up to 96 diagonals —
                    // three passes: 0.01 % of the rows have a third — and its cut, which is below its width; a wider row cannot be
                    // recorded: the unit is handed over.)
                    const uint32_t lo = hh ? (uint32_t)(fl0 >> 32) : (uint32_t)fl0, hi = NJ >= 2 ? (hh ? (uint32_t)(fl1 >> 32) : (uint32_t)fl1) : 0u;
                    const uint32_t top = NJ >= 3 ? (hh ? (uint32_t)(fl2 >> 32) : (uint32_t)fl2) : 0u;
                    if (NJ > 3) cns_bad = true;
                    ca.rowlog[logpos] = CnsRowRec{lo, hi, (uint32_t)last_ns | ((uint32_t)cut << 8), top};
                    logpos += 1;
                }
            }
        };
        // The next row of a half (nslot slots, at lin) must not store beyond the ring's end: where it would, the row starts at entry RING_ORG
        // instead.  The row that ran last stays where it is — pb_l and rlin_l point into it — and the three reserved entries take what a
        // reader needs to get from the relocated row to it (see the ring's description above).  The entry behind the last row is read
        // back from the ring: sepv describes the next row by now.  In front of every row outside the two fast loops, which leave
        // through ring_wraps for it.
        auto ring_relocate = [&]() __attribute__((always_inline)) {
            const unsigned int ext = max(twice((unsigned)nslot), ROW_STORE);      // what the row's passes store, see row_passes
            const bool need = lin_l + (ext - ROW_STORE) > wrap_l;
            if (BALLOT(need)) {
                if (need) {
                    const uint32_t rbase = RING_BASE(wrap_l), lin_u = lin_l - 2u * sl, off = lin_u - rbase;
                    lds_u32_t* const org = (lds_u32_t*)(uintptr_t)rbase;
                    const int behind = ring_ld(lin_u - 2u);
                    const uint32_t skew = (*org >> RING_LINK_BITS) + ((off - 2u * RING_ORG) >> 1);
                    if (sl == 0) { *org = (off - 2u) | (skew << RING_LINK_BITS); ring_st<4>(rbase, behind); }
                    lin_l = org_l;
                    nev += (inblock && sl == NEV_RELOC) ? 1u : 0u;
                }
                __builtin_amdgcn_wave_barrier();
            }
        };
        // a half's next row of one or two passes would not fit: all ones in the half's word of the compare, negative as one value
        auto ring_wraps = [&]() __attribute__((always_inline)) {
            const unsigned long long w = BALLOT(lin_l > wrap_l);
            return (int)(word_lo(w) | word_hi(w));
        };
        int ns_a = __builtin_amdgcn_readlane(nslot, 0), ns_b = __builtin_amdgcn_readlane(nslot, 32);
        if (inmask == ~0ull) {
            // Both halves in a block (98.6 % of the dual rows; it stays that way for as long as the loop runs): the band update writes
            // its per-half values without the `inblock` guard, and the loop control is scalar — the rows the two blocks may still run
            // (d < dlim in both) as one count-down, the band-size limits (:118 "max_k - min_k <= band_size") of the two halves next to
            // the slot counts, which are on the scalar unit anyway.  One-pass rows run in a loop of their own.
            const int rows_left = min(__builtin_amdgcn_readlane(dlim - d, 0), __builtin_amdgcn_readlane(dlim - d, 32));
            const int lim_a = (__builtin_amdgcn_readlane(band_tol2, 0) >> 1) + 1, lim_b = (__builtin_amdgcn_readlane(band_tol2, 32) >> 1) + 1;
            const int one_a = min(lim_a, 32), one_b = min(lim_b, 32);
            const int two_a = min(lim_a, 63), two_b = min(lim_b, 63);
            typedef std::integral_constant<int, 0> fast0;
            typedef std::integral_constant<int, 1> fast1;
            typedef std::integral_constant<int, 2> fast2;
            // Both halves advance by the same rows here and nothing in the loops reads d: the rows are counted on the scalar unit and
            // added to d once behind the loops (a per-lane d += go is a v_addc per row).  One counter does it: rows_more, the rows that
            // may run behind the current one, which is also the loops' bound; a row that reached an end marks it (snake_step_end).
            int rows_more = rows_left - 1;
            while (true) {
                // The two fast loops also run only while the next row of both halves fits in front of the ring's end (ring_wraps: one
                // vector compare and two scalar instructions per row, in the same sign test).  The rare exit comes by here, the half or
                // halves are relocated and the loops are entered again.
                ring_relocate();
                int wraps = 0;
                // one-pass rows (rows left, and both slot counts within their limits: one sign test)
                while ((rows_more | (one_a - ns_a) | (one_b - ns_b) | wraps) >= 0) {
                    DWS_ROW(~0ull, ns_a, ns_b, 1);
                    row_passes(1, ns_a, ns_b, rows_more, fast1{});     // (stores the entry behind a row of 32 slots itself)
                    lin_l += row_bytes;
                    band_update(1, last_m0, last_mp, std::true_type{}, ns_a, ns_b);
                    log_row(1, std::true_type{});
                    // (a row that reached an end leaves the loop through its bound, which snake_step_end has marked: a second exit makes
                    // the compiler build a machine of flag registers and re-tested branches around every row)
                    rows_more -= 1;
                    wraps = ring_wraps();
                    __builtin_amdgcn_wave_barrier();
                }
                if (ended) break;
                // two-pass rows: a half has 33 .. 63 slots
                while ((rows_more | (two_a - ns_a) | (two_b - ns_b) | (max(ns_a, ns_b) - 33) | wraps) >= 0) {      // (one sign test: rows left, slot counts within 33 .. limit)
                    DWS_ROW(~0ull, ns_a, ns_b, 2);
                    NJ = 2;
                    row_passes(2, ns_a, ns_b, rows_more, fast2{});
                    band_update(2, last_m0, last_mp, std::true_type{}, ns_a, ns_b);
                    log_row(2, std::true_type{});
                    lin_l += row_bytes;
                    rows_more -= 1;
                    wraps = ring_wraps();
                    __builtin_amdgcn_wave_barrier();
                }
                if (ended) break;
                if (rows_more < 0 || ns_a > lim_a || ns_b > lim_b) break;
                const int ns_max = max(ns_a, ns_b);
                if (ns_max < 64 || wraps < 0) continue;      // back to the two loops above, by way of the relocation
                // a half with 64 slots or more (0.01 % of the rows): the general form
                NJ = (ns_max + 31) >> 5;
                DWS_ROW(~0ull, ns_a, ns_b, NJ);
                row_passes(NJ, ns_a, ns_b, rows_more, fast0{});
                rows_more -= 1;
                lin_l += row_bytes;
                if ((ns_max & 31) == 0) ring_st(lin_l - 2u * sl - 2u, sepv);      // a half fills its last pass: no idle lane for the entry behind its row
                band_update(NJ, last_m0, last_mp, std::true_type{}, ns_a, ns_b);
                log_row(NJ, std::true_type{});
                if (ended) break;
                __builtin_amdgcn_wave_barrier();
            }
            // every exit of the loop comes by here: a row that reached an end is not counted (the end-of-block code below counts it)
            d += rows_left - 1 - rows_more_value(rows_more, ended != 0) - (ended ? 1 : 0);
        } else {
            // one half is between blocks (or out of units) while the other one rows on: the general form of everything
            const int slot_lim = (band_tol2 >> 1) + 1;
            int no_count = 0;      // (row_passes marks its caller's count-down when a row reaches an end: this loop has none and tests `ended`)
            while (true) {
                // the two conditions as masks (a ballot of their conjunction makes the compiler turn the mask into a 0/1 vector and
                // compare it again)
                const unsigned long long rmask = BALLOT(d < dlim) & BALLOT(nslot <= slot_lim);
                if (rmask != inmask) break;
                ring_relocate();      // (the half without a block too: its lanes store like the others, into a ring that nobody reads)
                const int ns_max = max(ns_a, ns_b);
                NJ = (ns_max + 31) >> 5;
                DWS_ROW(rmask, ns_a, ns_b, NJ);
                row_passes(NJ, ns_a, ns_b, no_count, std::integral_constant<int, 0>{});
                lin_l += row_bytes;
                if ((ns_max & 31) == 0) ring_st(lin_l - 2u * sl - 2u, sepv);
                band_update(NJ, last_m0, last_mp, std::false_type{}, ns_a, ns_b);
                log_row(NJ, std::false_type{});
                if (ended) break;
                d += 1;
                __builtin_amdgcn_wave_barrier();
            }
        }
        DWS_T(t_c);
        DWS_ADD(tk_rows, t_b, t_c);
#ifdef MECAT_DW_STATS
        n_ended += ended ? 1u : 0u;
#endif
        if (ended) {
            // Once per block, outside the row loop (inside it, the state written here costs register copies on every row): the
            // lowest diagonal that reached an end (:168-169), from the row just stored.  The band update for the row after it has been
            // done already (the other half goes on with it): the band of the end row is what that update started from — its slots
            // from the row's length in the ring, its first diagonal from the cut.
            // (mk_l is in doubled units and even: halved, it is the base-unit value the rest of the block's code works with)
            const int en = (int)((lin_l - rlin_l) >> 1) - 1, emk_l = (mk_l >> 1) - 2 * cut + 1;
            const int q_len = q_len2 >> 1, t_len = t_len2 >> 1;
            int hkey = 0x7fffffff;
            for (int j = 0; BALLOT(sl + 32 * j < en); ++j) {
                const int k = emk_l + 64 * j, kk = k + k_offset;
                if (sl + 32 * j < en) {
                    const int x = ring_ld(rlin_l + 64u * (unsigned)j) >> 1;     // (base units: hkey has ten bits for it)
                    if (x >= q_len || x - k >= t_len) hkey = min(hkey, (kk << 10) | x);
                }
            }
            hkey = half_min(hkey);
            if (inblock && hkey != 0x7fffffff) {
                end_k = (hkey >> 10) - k_offset; end_x = hkey & 1023; end_d = d;
                end_mk = emk_l - 2 * sl;
                dlim = 0;
            }
            d += 1;
            __builtin_amdgcn_wave_barrier();
        }
        row_ok = d < dlim && nslot <= (band_tol2 >> 1) + 1;
        DWS_T(t_d);
        DWS_ADD(tk_ended, t_c, t_d);

        const bool fin = inblock && !row_ok;

        // ---- 4. tail traceback == trim_mismatch_end(.., 4, ..) (gapalign.cpp:47-68), for the halves whose rows just ended
        bool has_aln = fin && end_d >= 0;
        // rows ran without reaching an end: needs the best point (dw_extend).  CNS: Align has failed, the direction ends (dw.cpp:302-304)
        bool handover = !CNS && fin && d > 0 && end_d < 0;
        const int end_y = end_x - end_k;
        const int aln_size = (end_x + end_y + end_d) / 2;
        int cd = end_d, ck = end_k, cx2 = 2 * end_x;      // cx2, acnt2: the walk's x and its column count in doubled units, like the ring's entries
        int acnt2 = 0, found = 0;
        bool tracing = CNS ? (has_aln && !last_block) : has_aln;      // (CNS: a last block keeps all of its columns, dw.cpp:353-358)
        // Rows are walked back over the entries between them: behind row r sits ~(slots of r | left cut of row r - 1 << 8).  clin / cmin:
        // ring position and first diagonal of row cd (the row that reached the end is the row that ran last); sepc: the entry behind row
        // cd — what a step reads in front of row cd (the entry behind row cd - 1) is that entry of the next step, so only the first one
        // is read here (the band update behind the end row has replaced the live copy of it).
        const unsigned int lin_u = lin_l - 2u * sl;
        unsigned int clin = rlin_l - 2u * sl;
        int cmin = end_mk;
        int sepc = ~ring_ld(lin_u - 2u);
        // Rows from the origin up to lin_u are of the current lap; once the walk has gone through the link it is in the lap before, whose rows
        // are whole while they lie ROW_STORE bytes or more ahead of lin_u (what the passes of the last row may have stored behind it).
        bool crossed = false;
        while (BALLOT(tracing)) {
            if (tracing) {
                // The path came to (cx2, diagonal ck) of row cd from diagonal ck - 1 (vl, one query base) or ck + 1 (vr, one target base)
                // of row cd - 1 and then ran along the snake from x1: x1 = max(vl + 1, vr), from the right when vl < vr, and the point it
                // left row cd - 1 at is x = max(vl, vr).  The walk's x values are doubled, as the ring holds them: + 1 is + 2, a run of four is
                // 8, and the counts are halved behind the loop.  A neighbour outside row cd - 1 counts as -1 (-2), which is all the reference's edge
                // tests (k == min_k: from the right; k == max_k: from the left) do: inside row cd - 1 but outside the band that row cd
                // was cut to, the left neighbour of min_k has vl + 1 < vr and the right neighbour of max_k vr < vl + 1 (see row_passes).
                // One straight line of selects (nested conditions cost a copy of every carried value per branch); in row 0 (cd == 0:
                // the snake runs back to x = 0), and in a step that finds the row lost, the ring reads are made and not used — LDS reads fault nowhere.
                const bool up = cd > 0;
                const int sp = ~ring_ld(clin - 2u);      // (a relocated row: the copy at entry 2)
                const int pcut = (sepc >> 8) & 127, pns = sp & 255;
                // the row in front ends at the entry in front of this row, or, for a row at the ring's origin (never row 0: `up`), where the link says
                const bool cross = (clin & (2u * RCAP - 1u)) == 2u * RING_ORG;
                // (the link: the low bits of the word at the origin, read in every step rather than kept in a register across the walk)
                const uint32_t link = *(lds_u32_t*)(uintptr_t)RING_BASE(clin) & (2u * RCAP - 1u);
                const unsigned int plin = (cross ? RING_BASE(clin) | link : clin - 2u) - 2u * (unsigned)pns;
                // the row in front has left the ring — it is in the lap before and the write point has come within ROW_STORE bytes of it (what the
                // idle lanes of the last row's passes may have written behind it, see row_passes; that bound also keeps the walk from a second
                // link: lin_u + ROW_STORE lies behind the origin) —, or its cut was 127 or more and is not recorded: the unit is handed over,
                // whatever else this step computes
                const bool over = crossed || cross;
                const bool lost = up && (pcut == 127 || (over && (int)(plin - lin_u) < (int)ROW_STORE));
                nev += (up && cross && sl == NEV_LINK) ? 1u : 0u;
                crossed = over;
                const int pmin = cmin - 2 * pcut + 1;
                // byte offsets of the two neighbours in row cd - 1 (two bytes per diagonal, diagonals two apart): one unsigned compare
                // each against the row's last offset
                const unsigned int ol = (unsigned)(ck - 1 - pmin), olast = 2u * (unsigned)pns - 2u;
                const int rl = ring_ld(plin + ol), rr = ring_ld<2>(plin + ol);
                const int vl = ol <= olast ? rl : -2, vr = ol + 2u <= olast ? rr : -2;      // (-1 in doubled units)
                const int x1 = up ? max(vl + 2, vr) : 0;
                const int sn = cx2 - x1;
                const bool run4 = sn >= 8;                       // the run of four matches: the walk ends in front of it
                const bool go = up && !run4 && !lost;            // otherwise one more row back (in row 0 there is none: no run found)
                acnt2 += run4 ? 8 : sn + (up ? 2 : 0);
                cx2 = run4 ? cx2 - 8 : (up ? max(vl, vr) : 0);
                ck = go ? ck + (vl < vr ? 1 : -1) : ck;
                cd -= go ? 1 : 0;
                found = run4 ? 1 : 0;
                clin = plin; cmin = pmin; sepc = sp;
                handover = handover || lost;
                tracing = go;
            }
        }
        // query / target bases the walk took off the end of the alignment: it stands at (cx, diagonal ck)
        const int cx = cx2 >> 1;
        int acnt = acnt2 >> 1;
        int qcnt = end_x - cx, tcnt = end_y - (cx - ck);
        const int trim_ok = has_aln && found && (aln_size - acnt >= 2);
        DWS_T(t_e);
        DWS_ADD(tk_trace, t_d, t_e);

        const int qblk = q_len2 >> 1, tblk = t_len2 >> 1;
        // ---- 5. block accounting (dw_in_one_direction, diff_gapalign.cpp:259-290); a block this kernel cannot finish (0.07 %: the
        // tail needs a row that left the ring, or no end was reached) hands the unit over to dw_extend, which redoes that block
        // and the rest of the unit with every row kept
        if (CNS && fin) {
            // dw_in_one_direction, dw.cpp:333-373.  A block that reached an end contributes the columns in front of its last run of four
            // matches (all of them when it is the direction's last block) and the next block starts there; a block without such a run, or
            // one that would contribute no query base, ends the direction without contributing.
            bool done = true;
            if (handover || cns_bad) {
                if (sl == 0) {
                    ca.hand_units[1u + atomicAdd(ca.hand_units, 1u)] = unit;
                    CnsDir D = {0, 0, 0, 0, 0, -1};
                    ca.dres[unit] = D;
                    nev += 1;
                }
            } else {
                nev += (sl == NEV_BLOCKS) ? 1u : 0u;
                nev += (sl == NEV_CELLS) ? ((lin_l - org_l - 6u) >> 1) + (*(lds_u32_t*)(uintptr_t)RING_BASE(wrap_l) >> RING_LINK_BITS) - (unsigned)d : 0u;
                bool keep = has_aln && (last_block || found);
                const int kept_q = end_x - qcnt, kept_t = end_y - tcnt, kept_cols = aln_size - acnt;      // (last block: nothing was walked)
                keep = keep && kept_q != 0;
                if (keep && Rc + kept_cols > ca.dir_cols_cap) { keep = false; if (sl == 0) atomicExch(ca.err_flag, 1); }
                if (keep && blkpos >= blkend) {
                    // the unit's share of block records ((ext >> 8) + 4, cns_caps) is used up — blocks that each advance by fewer than 256
                    // bases: like the other limits of the record format, the unit goes to cns_extend, which redoes it from its start
                    // (cns_trace skips the blocks of a handed-over unit)
                    if (sl == 0) {
                        ca.hand_units[1u + atomicAdd(ca.hand_units, 1u)] = unit;
                        CnsDir D = {0, 0, 0, 0, 0, -1};
                        ca.dres[unit] = D;
                        nev += 1;
                    }
                } else {
                    if (keep) {
                        if (sl == 0) {
                            CnsBlockRec B = {unit, qidx, tidx, qblk, end_d, end_k, end_mk, end_x, Rc, kept_cols, blk_log0, 0};
                            ca.blocks[blkpos] = B;
                        }
                        blkpos += 1;
                        Rc += kept_cols; Rq += kept_q; Rt += kept_t;
                        if (!last_block) { qidx += kept_q; tidx += kept_t; done = false; }
                    }
                    if (done && sl == 0) { CnsDir D = {Rc, Rq, Rt, 0, 0, 0}; ca.dres[unit] = D; }
                }
            }
            if (done) need_unit = true;
            inblock = false;
            setup = true;
            dlim = 0;
        }
        if (!CNS && fin) {
            bool stop;
            if (handover) {
                if (sl == 0) {
                    DwHandover h;
                    h.unit = unit; h.qidx = qidx; h.tidx = tidx;
                    h.R.qbases = Rq; h.R.tbases = Rt; h.R.matches = Rm; h.R.columns = Rc; h.R.blocks = Rb; h.R.pad = 0;
                    hand[atomicAdd(hand_count, 1u)] = h;
                    nev += 1;
                }
                need_unit = true;
            } else {
                nev += (sl == NEV_BLOCKS) ? 1u : 0u;
                // diagonals visited in this block (d rows, one -1 behind each): the entries from row 0 to lin, with those the relocations skipped
                nev += (sl == NEV_CELLS) ? ((lin_l - org_l - 6u) >> 1) + (*(lds_u32_t*)(uintptr_t)RING_BASE(wrap_l) >> RING_LINK_BITS) - (unsigned)d : 0u;
                Rb += 1;
                stop = !has_aln || !trim_ok;
                if (!stop) {
                    const int full_map = (qblk - end_x <= 20 || tblk - end_y <= 20);
                    const bool last = last_block || !full_map;
                    if (last) { qcnt -= 4; tcnt -= 4; acnt -= 4; }
                    Rc += (end_x + end_y + end_d) / 2 - acnt;
                    Rm += (end_x + end_y - end_d) / 2 - (qcnt + tcnt - acnt);
                    Rq += end_x - qcnt;
                    Rt += end_y - tcnt;
                    if (last) stop = true;
                    else { qidx += end_x - qcnt; tidx += end_y - tcnt; }
                }
                if (stop) {
                    if (sl == 0) { DirResult R = {Rq, Rt, Rm, Rc, Rb, 0}; dres[unit] = R; }
                    need_unit = true;
                }
            }
            inblock = false;
            setup = true;
            dlim = 0;           // a half without a block must never look like it is rowing (its rows may have ended on the band limit)
        }
        DWS_T(t_f);
        DWS_ADD(tk_acct, t_e, t_f);
    }
    unsigned long long c64 = sl == NEV_CELLS ? nev : 0u, b64 = sl == NEV_BLOCKS ? nev : 0u;
    unsigned long long h64 = sl == NEV_HAND ? nev : 0u, r64 = sl == NEV_RELOC ? nev : 0u, l64 = sl == NEV_LINK ? nev : 0u;
    for (int off = 32; off > 0; off >>= 1) { b64 += __shfl_xor(b64, off); c64 += __shfl_xor(c64, off); h64 += __shfl_xor(h64, off); r64 += __shfl_xor(r64, off); l64 += __shfl_xor(l64, off); }
    if (lane == 0) {
        atomicAdd(&counters[3], b64);
        atomicAdd(&counters[4], c64);
        atomicAdd(&counters[8], h64);          // units handed over
        atomicAdd(&counters[30], r64);         // rows relocated to the ring's origin
        atomicAdd(&counters[31], l64);         // tail-walk steps taken through a link
#ifdef MECAT_DW_STATS
        atomicAdd(&counters[9], nrows);          // dual rows
        atomicAdd(&counters[10], nidle);         // dual rows with one idle half
        atomicAdd(&counters[11], nwide);         // dual rows with more than 32 diagonals in a half
        atomicAdd(&counters[16], wall_clock64() - tk_start);      // wave life, ticks
        atomicAdd(&counters[17], tk_setup);
        atomicAdd(&counters[18], tk_rows);
        atomicAdd(&counters[19], tk_ended);
        atomicAdd(&counters[20], tk_trace);
        atomicAdd(&counters[21], tk_acct);
        atomicAdd(&counters[22], n_outer);
        atomicAdd(&counters[23], n_setup);
        atomicAdd(&counters[24], n_ended);
        atomicAdd(&counters[25], n_pass3);
        atomicAdd(&counters[26], 1ull);                           // waves
        atomicAdd(&counters[27], snake2);
        atomicAdd(&counters[28], n_one);
        atomicAdd(&counters[29], n_one32);
        for (int i = 0; i < 8; ++i) atomicAdd(&counters[32 + i], nh[i]);
        for (int i = 0; i < 6; ++i) atomicAdd(&counters[40 + i], q16[i]);
#endif
    }
}

int dw_extend2_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, DirResult* dres,
                      DwHandover* hand, unsigned int* hand_count, unsigned int* cursor) {
    int waves = DW2_WAVES_PER_SIMD * 4;                   // LDS 20 KB per four waves, 64 VGPRs
    if (const char* e = getenv("MECAT_DW_WAVES")) waves = std::max(4, std::min(32, atoi(e)));   // tuning/debug knob
    const int grid = std::min(c->num_cus * waves / AL_WAVES, (n + AL_WAVES - 1) / AL_WAVES);
    if (getenv("MECAT_TRACE")) {
        int nb = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dw_extend2<false>, AL_BLOCK, 0);
        fprintf(stderr, "[dw trace] occupancy query: %d blocks of %d threads per CU; grid %d; staged words %zu bytes per half\n", nb, AL_BLOCK, grid,
                sizeof(StagedLds) / (AL_WAVES * 2));
    }
    CnsFwdArgs none;
    memset(&none, 0, sizeof(none));
    LAUNCH(c, "dw_extend2", dw_extend2<false>, grid, AL_BLOCK, 0, (const uint32_t*)ref->d_pac, (const mhip_offset_t*)ref->d_offs,
           (const uint32_t*)reads->d_pac, (const mhip_offset_t*)reads->d_offs, (const mhip_aln_job*)d_jobs, n, dres, hand, hand_count,
           cursor, (unsigned long long*)c->d_counters, none);
    return 0;
}

// the forward pass of the mecat2cns re-aligner (cns_fwd.h): dw_extend2 under mecat2cns' block rules, with a cursor of its own
int cns_forward_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, const CnsFwdArgs& args) {
    unsigned int* d_cur;
    if (c->scratch("cnf_cursor", 64, (void**)&d_cur)) return -1;
    HIPCHK(hipMemsetAsync(d_cur, 0, 16, c->stream));
    const int waves = getenv("MECAT_CNS_WAVES") ? std::max(4, std::min(32, atoi(getenv("MECAT_CNS_WAVES")))) : 4 * CNS_FWD_WAVES_PER_SIMD;
    const int grid = std::min(c->num_cus * waves / AL_WAVES, (n + AL_WAVES - 1) / AL_WAVES);
    CnsFwdArgs a = args;
    a.full_max_d = (int)(2.0 * a.error_rate * (SEG_BLK + SEG_BLK));      // the block set-up's expression at qblk = SEG_BLK
    LAUNCH(c, "cns_forward", dw_extend2<true>, grid, AL_BLOCK, 0, (const uint32_t*)ref->d_pac, (const mhip_offset_t*)ref->d_offs,
           (const uint32_t*)reads->d_pac, (const mhip_offset_t*)reads->d_offs, (const mhip_aln_job*)d_jobs, n, (DirResult*)nullptr,
           (DwHandover*)nullptr, (unsigned int*)nullptr, d_cur, (unsigned long long*)c->d_counters, a);
    return 0;
}
