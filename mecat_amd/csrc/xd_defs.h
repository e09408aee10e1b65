// xd_defs.h — what the parts of the X-drop aligner share (xalign.hip, xd_block_ring.h, xd_block_wide.h, xd_order.hip): the reference's
// parameters, the per-direction result, a block's result with the trim-tail bookkeeping that fills it, the constants of the two block
// formulations, the DPP scans of a row, and the prototype of the longest-first sort.
#pragma once
#include "common.h"

#define X_SEG 500
#define X_MAXN 736                       // last block: one side < 600, the other <= 718 (gapalign.cpp:24-30)
#define X_MIN_SCORE (-100000000)

enum { XS_SUB = 3, XS_GAP_IN_A = 0, XS_GAP_IN_B = 6, XS_OP_MASK = 0x07, XS_EXT_A = 0x10, XS_EXT_B = 0x40 };   // xdrop_gapalign.h:13-34

struct XDir {
    int32_t qbases, tbases, matches, columns;     // kept alignment of one direction
    int32_t last_q, last_t, last_m;               // type of its LAST column (the left half drops it, xdrop_gapalign.cpp:401-402)
    int32_t blocks;
};

struct XView {
    const uint32_t* pac;
    int64_t off;
    int A, B, comp;     // logical position i -> volume base off + A + B * i, complemented if comp
};
__device__ __forceinline__ int xv_at(const XView& v, int i) {
    const uint32_t c = pac_base(v.pac, v.off + v.A + (int64_t)v.B * i);
    return (int)(v.comp ? 3u - c : c);
}

// A block's two template parameters.  The sequence view: any type V with xv_at(const V&, int) -> code of logical base i (XView below is
// mecat2pw's: a read of a volume, whole-read complement).  The column sink: told every gap column the traceback meets, as
// gap(i, code) with i = the column's place counted from the block's TAIL (the walk's order, 0 = the last column of the block's
// strings) and code 1 = target base only, 2 = query base only; wave-uniform.  Substitution columns are not reported: their number
// follows from XBlockOut::n.  XNoSink keeps nothing (mecat2pw needs counts only).
struct XNoSink {
    __device__ __forceinline__ void gap(int, int) const {}
};

struct XBlockOut {
    int ae, be;                 // aln_qe, aln_te
    int n, nmatch;              // alignment columns / equal columns of the block
    int qcnt, tcnt, acnt, mtail;// trim_mismatch_end: bases/columns/equal columns from the tail through the 4-match run
    int trim_ok;
    int l0q, l0t, l0m;          // type of the last column of the whole block string
    int l1q, l1t, l1m;          // type of the column just before the trimmed tail
    int overflow;
    int cells, rows;            // work counters: DP cells visited (window widths summed over the rows), rows
#ifdef MECAT_XD_STATS
    unsigned long long tk_stage, tk_rows, tk_trace, n_rows2, n_win, n_steps, n_qfill;      // section clocks (s_memtime ticks) and event counts of the block
#endif
};
__device__ __forceinline__ void xblock_clear(XBlockOut& o) {
    o.ae = o.be = 0; o.n = o.nmatch = 0; o.qcnt = o.tcnt = o.acnt = o.mtail = 0; o.trim_ok = 0; o.overflow = 0;
    o.l0q = o.l0t = o.l0m = o.l1q = o.l1t = o.l1m = 0;
    o.cells = o.rows = 0;
#ifdef MECAT_XD_STATS
    o.tk_stage = o.tk_rows = o.tk_trace = o.n_rows2 = o.n_win = o.n_steps = o.n_qfill = 0;
#endif
}

// section clocks and event counts of a block (make xdstats); `o` is the block's XBlockOut, `tk0` the clock at the section's start
#ifdef MECAT_XD_STATS
#define XD_TICK(field) do { const unsigned long long _t = __builtin_amdgcn_s_memtime(); o.field += _t - tk0; tk0 = _t; } while (0)
#define XD_COUNT(field) (++o.field)
#else
#define XD_TICK(field) do { } while (0)
#define XD_COUNT(field) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------------------------
// XTail — what a traceback keeps while it walks from the block's end (the alignment's tail) towards its start: the columns and equal
// columns so far, the tail's first run of four matches (trim_mismatch_end: the walk's state right after it) and the column types the
// stitching needs.  A column's type is packed as q | t << 1 | match << 2 (1: the column takes a query base, 2: a target base).
// The wide block feeds it column by column (step).  The ring block takes a turn's columns at once: it gives the first one's type
// (column_type), the streak through a run of substitutions (run) and the gap column behind it (gap_after_run), and adds the turn's
// columns to n and nmatch itself — that addition is all its lean second loop does.  Both end with finish.
struct XTail {
    int n = 0, nmatch = 0;                               // columns, equal columns
    int m = 0, found = 0;                                // the current streak of matches; the first run of four was seen
    int want_l1 = 0, first = 0, l1 = 0;                  // the next column is the one before the trimmed tail; type of the first column, of that one
    int sn_n = 0, sn_a = 0, sn_b = 0, sn_m = 0;          // the walk's state right after the first run of 4 matches

    // the type of the column that comes next: the block's first, the one before the trimmed tail
    __device__ __forceinline__ void column_type(int pk) {
        first = n == 0 ? pk : first;
        l1 = want_l1 ? pk : l1;
        want_l1 = 0;
    }
    // one column; (a_after, b_after): the walk's position behind it
    __device__ __forceinline__ void step(int cq, int ct, int cm, int a_after, int b_after) {
        column_type(cq | (ct << 1) | (cm << 2));
        ++n;
        nmatch += cm;
        m = cm ? m + 1 : 0;
        if (m == 4 && !found) { found = 1; want_l1 = 1; sn_n = n; sn_a = a_after; sn_b = b_after; sn_m = nmatch; }
    }
    // the streak through r >= 1 substitution columns at once, bit i of Mbits: column i is a match (no bits from r on); (a_before,
    // b_before): the walk's position in front of them.  The caller has given the first column's type and counts the columns itself
    // (n += r, nmatch += popcount: all that the ring's lean loop does).
    __device__ __forceinline__ void run(int r, uint32_t Mbits, int a_before, int b_before) {
        const uint32_t mask = r >= 32 ? 0xffffffffu : ((1u << r) - 1u);
        const uint32_t inv = ~Mbits & mask;                                // the mismatches of the run
        if (!found) {
            const int z = inv ? __builtin_ctz(inv) : r;                    // leading matches
            int hit = -1;                                                  // the column at which the streak first reaches 4
            if (m + z >= 4) hit = 3 - m;
            else {
                const uint32_t Q = Mbits & (Mbits >> 1) & (Mbits >> 2) & (Mbits >> 3);
                if (Q) hit = __builtin_ctz(Q) + 3;
            }
            if (hit >= 0) {
                found = 1;
                sn_n = n + hit + 1; sn_a = a_before - (hit + 1); sn_b = b_before - (hit + 1);
                sn_m = nmatch + __builtin_popcount(Mbits & ((2u << hit) - 1u));
                if (hit + 1 < r) l1 = 3 | (int)(((Mbits >> (hit + 1)) & 1u) << 2);
                else want_l1 = 1;
            }
        }
        m = inv ? r - 1 - (31 - __builtin_clz(inv)) : m + r;               // matches after the last mismatch
    }
    // the gap column behind a run, taken in the same turn (never the block's first column)
    __device__ __forceinline__ void gap_after_run(int gq, int gt) {
        l1 = want_l1 ? (gq | (gt << 1)) : l1;
        want_l1 = 0;
        m = 0;
        ++n;
    }
    // the walk ended: (ae, be) is where it began
    __device__ __forceinline__ void finish(int ae, int be, XBlockOut& o) const {
        o.n = n; o.nmatch = nmatch;
        o.l0q = first & 1; o.l0t = (first >> 1) & 1; o.l0m = first >> 2;
        o.l1q = l1 & 1; o.l1t = (l1 >> 1) & 1; o.l1m = l1 >> 2;
        o.acnt = found ? sn_n : n; o.qcnt = found ? ae - sn_a : ae; o.tcnt = found ? be - sn_b : be; o.mtail = found ? sn_m : nmatch;
        o.trim_ok = found && (n - o.acnt >= 2);
    }
};

// ---- constants of the two block formulations
#define XW_WAVES 4
#define XW_BLOCK (XW_WAVES * 64)
#define XW_RING 128                      // ring block: cells of a row's scores in LDS
#define XW_ROWCELLS 128                  // ring block: script cells of a row (two chunks of 64); a row wider than XW_ROWCELLS - 2 overflows
#define XW_WIN 4096                      // wide block: bytes of the traceback's LDS window over the script rows
#define XW_WSTRIDE 768                   // wide block: script bytes per row; any window fits (N + 1 <= 737 cells)
#define XW_WIDE_BYTES ((size_t)(X_MAXN + 2) * XW_WSTRIDE)
#define XW_WIDE_HF (X_MAXN + 8)
#define XW_INPLACE_STATE 16384           // bytes in front of a ring wave's wide rows: its XwWide image
#define XW_INPLACE_BYTES (XW_INPLACE_STATE + XW_WIDE_BYTES)
#define XW_NEG (-(1 << 30))
#define XS_MATCH 0x80
static_assert(XW_ROWCELLS <= XW_RING, "a row's script cells are cells of the ring");
static_assert(XW_WSTRIDE >= X_MAXN + 1 && XW_WIDE_HF >= X_MAXN + 1, "a wide row and the wide score array hold every cell of a block");
static_assert(XW_WIN % 256 == 0, "the wide traceback's window is loaded in rounds of one dword per lane");

template <int CTRL, int RMASK> __device__ __forceinline__ int xw_dpp_max(int v) {
    // old = the identity of max: lets the DPP combiner fuse mov_dpp + max into one v_max_i32_dpp and schedule around the hazard
    return max(v, __builtin_amdgcn_update_dpp((int)0x80000000, v, CTRL, RMASK, 0xf, false));
}
__device__ __forceinline__ int xw_scan_max(int v) {          // inclusive prefix max over the 64 lanes, all lanes active
    v = xw_dpp_max<0x111, 0xf>(v);                            // row_shr:1,2,4,8
    v = xw_dpp_max<0x112, 0xf>(v);
    v = xw_dpp_max<0x114, 0xf>(v);
    v = xw_dpp_max<0x118, 0xf>(v);
    v = xw_dpp_max<0x142, 0xa>(v);                            // row_bcast:15 into rows 1 and 3
    v = xw_dpp_max<0x143, 0xc>(v);                            // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ int xw_shr1(int v, int fill) {    // lane l gets lane l-1, lane 0 gets fill
    return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false);   // wave_shr:1
}

// xd_order.hip — longest first: *d_order = the jobs [0, n) in descending order of their reach (a stable sort, so a read's jobs stay
// neighbours), or NULL where sorting does not pay (no more jobs than the `waves` resident waves) or cannot be done
int xd_order_jobs(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, int waves, unsigned int** d_order);
