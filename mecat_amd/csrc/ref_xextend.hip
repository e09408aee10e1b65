// ref_xextend.hip — mecat2ref, stage 2 in nanopore mode (`-x 1`): every listed candidate through XdropAligner::go on the device, with the
// two aligned strings as 2-bit columns.  The technology changes one thing in the tool: reference_mapping creates an XdropAligner
// instead of a DiffAligner (mecat2ref/mecat2ref_impl_large.cpp:328-335); jobs, windows, slices and the fetch are ref_extend.hip's.
//
// Replaces, for the jobs ref_extend.hip's ref_jobs makes:
//   XdropAligner::go          common/xdrop_gapalign.cpp:359-439   left + right extension from the start point, the left half without its
//                                                                 last column (:401-402), ok = query span >= min_aln_size (:438)
//   align_ex                  common/xdrop_gapalign.cpp:263-357   blocks of 500, the last one by retrieve_next_aln_block, full_map,
//                                                                 trim_mismatch_end with a 4-match tail; a failed trim ends the direction
//                                                                 and drops the block
//   xdrop_align + script_to_aligned_string  :10-261               the block: xd_block_ring.h / xd_block_wide.h, the code mecat2pw's
//                                                                 xd_extend_w runs, instantiated with this file's view and sink
// One wave per (job, direction), persistent on a cursor.  What differs from xd_extend_w is what is kept: every gap column of a block's
// traceback goes into a per-wave LDS buffer of 2-bit codes in the walk's order (tail to head; XColSink), and once the block's kept part
// is known (XBlockOut::n and acnt) the wave appends it, reversed into extension order, at the direction's 2-bit offset in the column
// store.  Codes are stage 2's: 0 = both bases (a match OR a mismatch: X-drop paths have substitutions over unequal bases, the host tells
// them apart by the letters), 1 = target base only, 2 = query base only.
// Views (ref_extend.hip's rules): the target is the reference volume by absolute base position (no pad bases, non-ACGT stored as code
// 0); the query is the read on the candidate's strand, and on the reverse strand a base whose N-plane entry is set keeps its stored code
// while every other base is complemented.
// A block whose window outgrows the ring is redone at once with the wide block on the wave's global state, as in xd_extend_w's in-place
// arrangement; MECAT_XD_WIDE=1 sends every block that way (the cross-check).  Nothing here is tuned: see profiles/ref_xextend.md.
#include <stdlib.h>

#include <algorithm>

#include "ref_extend.h"
#include "xd_defs.h"

namespace {

// a sequence in extension order: logical base i is volume base off + B * i; comp: complemented unless its plane entry is set
struct RxSeq {
    const uint32_t* pac;
    const uint32_t* npac;        // the N-plane of the reads volume (NULL: none, and always for the reference)
    int64_t off;
    int B, comp;
};
__device__ __forceinline__ int xv_at(const RxSeq& v, int i) {
    const int64_t p = v.off + (int64_t)v.B * i;
    const uint32_t c = pac_base(v.pac, p);
    if (!v.comp) return (int)c;
    const uint32_t n = v.npac ? pac_base(v.npac, p) : 0u;
    return (int)(n ? c : 3u - c);
}

#define RXX_COL_WORDS ((2 * X_MAXN + 15) / 16)       // a block has at most X_MAXN + X_MAXN columns: 92 words of 2-bit codes

// the block's gap columns in the walk's order: column i from the tail at bits 2 (i & 15) of word i >> 4
struct XColSink {
    uint32_t* w;                 // RXX_COL_WORDS words of LDS, zero between blocks
    __device__ __forceinline__ void gap(int i, int code) const {
        if (lane_id() == 0) w[i >> 4] |= (uint32_t)code << ((i & 15) << 1);
    }
};

}  // namespace

#include "xd_block_ring.h"
#include "xd_block_wide.h"

namespace {

struct RxxLds {
    XrLds ring;
    uint32_t cols[RXX_COL_WORDS];
};

// units [u0, u1) (unit = 2 * slot + direction, 0 = left); the columns of unit u start at word dbase[u] - dbase[u0] of dstore (zero-filled)
__global__ __launch_bounds__(XW_BLOCK, 4) void ref_xextend(const uint32_t* __restrict__ rpac, const uint32_t* __restrict__ qpac,
                                                           const uint32_t* __restrict__ qnpac, const mhip_offset_t* __restrict__ qoffs,
                                                           const RxJob* __restrict__ jobs, unsigned int u0, unsigned int u1,
                                                           const unsigned long long* __restrict__ dbase, uint32_t* __restrict__ dstore,
                                                           RxDir* __restrict__ dres, uint8_t* __restrict__ scratch, uint8_t* __restrict__ wide_state,
                                                           int all_wide, unsigned int* __restrict__ cursor, unsigned int* __restrict__ redone,
                                                           unsigned long long* __restrict__ counters) {
    __shared__ RxxLds lds[XW_WAVES];
    RxxLds& S = lds[threadIdx.x >> 6];
    const int lane = lane_id();
    const size_t wave = (size_t)blockIdx.x * XW_WAVES + (threadIdx.x >> 6);
    uint8_t* st = scratch + wave * XR_STATE_BYTES;
    uint8_t* wst = wide_state + wave * XW_INPLACE_BYTES;
    const unsigned long long base0 = dbase[u0];
    unsigned long long nblocks = 0;
    unsigned int nredone = 0;
    const XColSink sink = {S.cols};
    for (int i = lane; i < RXX_COL_WORDS; i += 64) S.cols[i] = 0u;
    __builtin_amdgcn_wave_barrier();
    while (true) {
        unsigned int unit = 0;
        if (lane == 0) unit = atomicAdd(cursor, 1u);
        unit = __builtin_amdgcn_readfirstlane(unit) + u0;
        if (unit >= u1) break;
        const RxJob jb = jobs[unit >> 1];
        const int right = unit & 1;
        RxDir R = {0, 0, 0, 0};
        if (!jb.valid) { if (lane == 0) dres[unit] = R; continue; }
        // extension views: logical position i of the query is strand position read_start + i (right) or read_start - 1 - i (left); strand
        // position p of the reverse strand is original index read_len - 1 - p; the target is the concatenated reference itself
        const int qs0 = right ? jb.read_start : jb.read_start - 1, step = right ? 1 : -1;
        RxSeq q, t;
        q.pac = qpac; q.npac = qnpac; q.comp = jb.chain;
        q.off = qoffs[jb.rid].offset + (jb.chain ? jb.read_len - 1 - qs0 : qs0);
        q.B = jb.chain ? -step : step;
        t.pac = rpac; t.npac = nullptr; t.comp = 0;
        t.off = right ? jb.ref_start : jb.ref_start - 1;
        t.B = step;
        const int query_size = right ? jb.read_len - jb.read_start : jb.read_start;
        const int target_size = right ? jb.right : jb.left;
        uint32_t* uops = dstore + (size_t)(dbase[unit] - base0);
        int qidx = 0, tidx = 0, cols = 0;
        int last_q = 0, last_t = 0;                      // type of the direction's last column
        while (true) {      // align_ex (xdrop_gapalign.cpp:291-356)
            const int qleft = query_size - qidx, tleft = target_size - tidx;
            int qblk, tblk, last_block;
            if (qleft < X_SEG + 100 || tleft < X_SEG + 100) {
                qblk = min(qleft, (int)(tleft + tleft * 0.2));
                tblk = min(tleft, (int)(qleft + qleft * 0.2));
                last_block = 1;
            } else { qblk = X_SEG; tblk = X_SEG; last_block = 0; }
            XBlockOut o;
            bool wide = all_wide != 0;
            if (!wide) {
                xdrop_block_ring(S.ring, q, qidx, qblk, t, tidx, tblk, st, o, sink);
                if (o.overflow) {                        // (the ring's traceback has not run: the sink is still empty)
                    wide = true;
                    ++nredone;
                }
            }
            if (wide) xdrop_block_wide(*reinterpret_cast<XwWide*>(wst), q, qidx, qblk, t, tidx, tblk, wst + XW_INPLACE_STATE, o, sink);
            ++nblocks;
            R.blocks += 1;
            const int full_map = (qblk - o.ae <= 20 || tblk - o.be <= 20);
            const int whole = !full_map || last_block;
            const int keep = whole ? o.n : (o.trim_ok ? o.n - o.acnt : 0);
            // ---- the kept columns, reversed into extension order, at column `cols` of the direction: column j of the block is the
            // walk's column o.n - 1 - j.  Whole words from all lanes; the store is zero-filled and this wave alone writes the direction,
            // so a word shared with the block before is ORed into.
            __builtin_amdgcn_wave_barrier();
            if (keep > 0) {
                const int w0 = cols >> 4, w1 = (cols + keep - 1) >> 4;
                for (int w = w0 + lane; w <= w1; w += 64) {
                    uint32_t v = 0;
#pragma unroll
                    for (int b = 0; b < 16; ++b) {
                        const int j = 16 * w + b - cols;
                        if (j >= 0 && j < keep) {
                            const int s = o.n - 1 - j;
                            v |= ((S.cols[s >> 4] >> ((s & 15) << 1)) & 3u) << (b << 1);
                        }
                    }
                    if (v) atomicOr(&uops[w], v);
                }
            }
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < RXX_COL_WORDS; i += 64) S.cols[i] = 0u;
            __builtin_amdgcn_wave_barrier();
            if (whole) {
                if (o.n > 0) { cols += o.n; R.qbases += o.ae; R.tbases += o.be; last_q = o.l0q; last_t = o.l0t; }
                break;
            }
            if (!o.trim_ok) break;
            if (keep > 0) { cols += keep; R.qbases += o.ae - o.qcnt; R.tbases += o.be - o.tcnt; last_q = o.l1q; last_t = o.l1t; }
            qidx += o.ae - o.qcnt;
            tidx += o.be - o.tcnt;
        }
        // go leaves the left half's last column out (:401-402): it stays in the store behind the direction's columns, where nothing reads it
        if (!right && cols > 0) { cols -= 1; R.qbases -= last_q; R.tbases -= last_t; }
        R.cols = cols;
        if (lane == 0) dres[unit] = R;
    }
    if (lane == 0) {
        atomicAdd(&counters[3], nblocks);
        if (nredone) atomicAdd(redone, nredone);
    }
}

}  // namespace

int ref_xextend_launch(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const RxJob* d_jobs, unsigned int u0, unsigned int u1,
                       const unsigned long long* d_dbase, uint32_t* d_store, RxDir* d_dres, unsigned int* d_cursor, unsigned int* d_redone) {
    if (u1 <= u0) return 0;
    const char* e = getenv("MECAT_XD_WIDE");
    const int all_wide = e && atoi(e) == 1;
    // 8 waves per CU: every wave owns XW_INPLACE_BYTES of wide state in global memory besides its ring rows
    const int max_waves = c->num_cus * 8;
    const int grid = std::max(1, std::min(max_waves / XW_WAVES, (int)((u1 - u0 + XW_WAVES - 1) / XW_WAVES)));
    const size_t launched = (size_t)grid * XW_WAVES;
    uint8_t *d_s, *d_wst;
    if (c->scratch("rxx_state", XR_STATE_BYTES * launched, (void**)&d_s)) return -1;
    if (c->scratch("rxx_inplace", XW_INPLACE_BYTES * launched, (void**)&d_wst)) return -1;
    LAUNCH(c, "ref_xextend", ref_xextend, grid, XW_BLOCK, 0, (const uint32_t*)ref->d_pac, (const uint32_t*)reads->d_pac, (const uint32_t*)reads->d_npac,
           (const mhip_offset_t*)reads->d_offs, d_jobs, u0, u1, d_dbase, d_store, d_dres, d_s, d_wst, all_wide, d_cursor, d_redone,
           (unsigned long long*)c->d_counters);
    return 0;
}
