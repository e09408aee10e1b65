// xalign.hip — BLAST-style affine X-drop gapped extension in 500-bp blocks, the nanopore-mode aligner
// (used by mecat2pw -x 1 -j 1).
//
// Replaces XdropAligner::go (common/xdrop_gapalign.cpp:359-439), align_ex (:263-357), xdrop_align (:10-213) and
// script_to_aligned_string (:215-261) with reward 1, penalty -1, gap_open 0, gap_extend 1, X = 30, block 500
// (common/xdrop_gapalign.h:98-114).
//
// One WAVE per (candidate, direction) unit, lanes = cells of a row of the dynamic program (xd_extend_w below).  As in dw, only
// what mecat2pw consumes is produced: end coordinates and identity counts; the traceback walks the script once and does
// trim_mismatch_end and the match/column counting on the fly (XTail, xd_defs.h).  Two formulations of the same row exist, one file
// each: the RING block (xd_block_ring.h: 128-cell LDS ring, 4-bit script cells, run-by-run traceback — the default) and the WIDE block
// (xd_block_wide.h: scores indexed by b, 768-byte rows, byte-by-byte traceback) that takes over the blocks whose window outgrows the
// ring.  Three arrangements of the two: in place (default), hand-over (MECAT_XD_HANDOVER=1) and all-wide (MECAT_XD_WIDE=1), see
// xd_extend_w; tests/test_gpu_xalign.py compares all three (the sequential restatement they are checked against is test
// infrastructure, not part of this library).  The longest-first order of the jobs is xd_order.hip.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "aln_jobs.h"
#include "common.h"
#include "xd_defs.h"
#include "xd_block_ring.h"
#include "xd_block_wide.h"

// ------------------------------------------------------------------------------------------------------------------
// xd_extend_w — one WAVE per (candidate, direction).  A row of the dynamic program is per-cell independent work plus two
// prefix-max scans over the window (the tests check the equivalence with the sequential row state by state):
//   diag_b = H'[b-1] + s(A_a, B_{b-1}) (MIN for the row's first cell),  M_b = max(diag_b, F'[b]),
//   E_b = max_{j<b}(M_j + j) - b,  H_b = max(M_b, E_b),  best_b = max(best, max_{j<b} H_j),  dropped <=> best_b - H_b > X;
// a value carried across a dropped cell is below every later kept cell's score, so it only shows in the op bits of dropped
// cells (there E = H of the nearest kept cell to the left - 1, no decay).  Lanes = 64 consecutive cells, a second chunk with
// scalar carries when the window is wider.
// xd_extend_w<false>, the production kernel, runs every block in the ring.  A block whose window grows wider than XW_RING - 2 cells
// is redone at once by the same wave with the wide block — with its whole state (scores, bases, row starts, window) in the wave's share
// of a global buffer (wide_state) instead of LDS: slower per row, but only a fraction of a percent of the units (low-complexity
// sequence) have such a block, and the unit then goes on in the ring.  That is the IN-PLACE arrangement.
// Without wide_state (HAND-OVER, MECAT_XD_HANDOVER=1) such a unit is written to an overflow list instead — unit, position and partial
// result — and a second launch, xd_extend_w<true> with that list as ulist, runs the rest of the unit's blocks through the wide block
// in LDS.  (This was the default once: the second launch is as long as its slowest unit, 17.6 ms of 136 on 134 k jobs.)
// ALL-WIDE (MECAT_XD_WIDE=1) is xd_extend_w<true> alone on every unit: the ring's cross-check at scale.
template <bool WIDE>
__global__ __launch_bounds__(XW_BLOCK, 6) void xd_extend_w(const uint32_t* __restrict__ rpac, const mhip_offset_t* __restrict__ roffs,
                                                        const uint32_t* __restrict__ qpac, const mhip_offset_t* __restrict__ qoffs,
                                                        const mhip_aln_job* __restrict__ jobs, int n, XDir* __restrict__ dres,
                                                        uint8_t* __restrict__ scratch, unsigned int* __restrict__ cursor,
                                                        unsigned int* __restrict__ ovf_list, unsigned long long* __restrict__ counters,
                                                        const unsigned int* __restrict__ ulist, unsigned int nunits,
                                                        uint8_t* __restrict__ wide_state, const unsigned int* __restrict__ order) {
    __shared__ typename std::conditional<WIDE, XwWide, XrLds>::type lds[WIDE ? 1 : XW_WAVES];
    auto& S = lds[threadIdx.x >> 6];
    const int lane = lane_id();
    uint8_t* st = scratch + (size_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * (WIDE ? XW_WIDE_BYTES : XR_STATE_BYTES);
    // the ring kernel's own wide state (a block whose window outgrows the ring is redone in place, below): in global memory
    uint8_t* wst = WIDE ? nullptr : wide_state + (size_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * XW_INPLACE_BYTES;
    unsigned long long nblocks = 0, ncells = 0, nrows = 0, nredone = 0;
#ifdef MECAT_XD_STATS
    unsigned long long xs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long tk_life = __builtin_amdgcn_s_memtime();
#endif
    while (true) {
        unsigned int unit = 0;
        if (lane == 0) unit = atomicAdd(cursor, 1u);
        unit = __builtin_amdgcn_readfirstlane(unit);
        if (unit >= nunits) break;
        if (order) unit = (order[unit >> 1] << 1) | (unit & 1u);          // (jobs longest first)
        int qidx = 0, tidx = 0;
        XDir R = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ulist) {                                     // a handed-over unit resumes at the block that overflowed
            const unsigned int* e = ulist + 3 * (size_t)unit;
            unit = e[0]; qidx = (int)e[1]; tidx = (int)e[2];
            R = dres[unit];
        }
        const mhip_aln_job jb = jobs[unit >> 1];
        const int right = unit & 1;
        const int qsize = qoffs[jb.qid_local].size, tsize = roffs[jb.sid_local].size;
        XView q, t;
        q.pac = qpac; q.off = qoffs[jb.qid_local].offset; q.comp = jb.chain;
        t.pac = rpac; t.off = roffs[jb.sid_local].offset; t.comp = 0;
        const int qs0 = right ? jb.qstart : jb.qstart - 1, step = right ? 1 : -1;
        if (jb.chain) { q.A = qsize - 1 - qs0; q.B = -step; } else { q.A = qs0; q.B = step; }
        t.A = right ? jb.sstart : jb.sstart - 1; t.B = step;
        // (a start point in front of a read — the reference's wrapped seed numbers, pw_impl.cpp:388 — is a job without extension)
        const bool dead = jb.qstart < 0 || jb.sstart < 0;
        const int query_size = dead ? 0 : (right ? qsize - jb.qstart : jb.qstart);
        const int target_size = dead ? 0 : (right ? tsize - jb.sstart : jb.sstart);
        bool handed_over = false;
        while (true) {      // align_ex (xdrop_gapalign.cpp:263-357)
            const int qleft = query_size - qidx, tleft = target_size - tidx;
            int qblk, tblk, last_block;
            if (qleft < X_SEG + 100 || tleft < X_SEG + 100) {
                qblk = min(qleft, (int)(tleft + tleft * 0.2));
                tblk = min(tleft, (int)(qleft + qleft * 0.2));
                last_block = 1;
            } else { qblk = X_SEG; tblk = X_SEG; last_block = 0; }
            XBlockOut o;
            if constexpr (WIDE) xdrop_block_wide(S, q, qidx, qblk, t, tidx, tblk, st, o);
            else {
                xdrop_block_ring(S, q, qidx, qblk, t, tidx, tblk, st, o);
#ifdef MECAT_XD_STATS
                xs[0] += o.tk_stage; xs[1] += o.tk_rows; xs[2] += o.tk_trace; xs[3] += o.n_rows2; xs[4] += o.n_win; xs[5] += o.n_steps; xs[6] += o.n_qfill;
#endif
            }
            ++nblocks;
            R.blocks += 1;
            ncells += (unsigned)o.cells;
            nrows += (unsigned)o.rows;
            if constexpr (!WIDE) {
                if (o.overflow) {
                    // A window wider than the ring: the block again, at once, with the wide block on this wave's global state, rows of
                    // XW_WSTRIDE bytes behind it; the unit then goes on in the ring.
                    if (wst) {
                        xdrop_block_wide(*reinterpret_cast<XwWide*>(wst), q, qidx, qblk, t, tidx, tblk, wst + XW_INPLACE_STATE, o);
                        ncells += (unsigned)o.cells;
                        nrows += (unsigned)o.rows;
                        ++nredone;
                    } else { handed_over = true; R.blocks -= 1; break; }      // (no wide state: the block is counted again when it is redone)
                }
            }
            const int full_map = (qblk - o.ae <= 20 || tblk - o.be <= 20);
            if (!full_map || last_block) {
                if (o.n > 0) {
                    R.columns += o.n; R.matches += o.nmatch; R.qbases += o.ae; R.tbases += o.be;
                    R.last_q = o.l0q; R.last_t = o.l0t; R.last_m = o.l0m;
                }
                break;
            }
            if (!o.trim_ok) break;
            const int kept = o.n - o.acnt;
            if (kept > 0) {
                R.columns += kept; R.matches += o.nmatch - o.mtail; R.qbases += o.ae - o.qcnt; R.tbases += o.be - o.tcnt;
                R.last_q = o.l1q; R.last_t = o.l1t; R.last_m = o.l1m;
            }
            qidx += o.ae - o.qcnt;
            tidx += o.be - o.tcnt;
        }
        if (lane == 0) {
            dres[unit] = R;                              // final, or the state in front of the block that overflowed
            if (handed_over) {
                unsigned int* e = ovf_list + 1 + 3 * (size_t)atomicAdd(ovf_list, 1u);
                e[0] = unit; e[1] = (unsigned int)qidx; e[2] = (unsigned int)tidx;
            }
        }
    }
    if (lane == 0) {
        atomicAdd(&counters[3], nblocks);
        atomicAdd(&counters[4], ncells);      // DP cells (the slot dw's d-path cells use)
        atomicAdd(&counters[32], nrows);                     // slots 32 / 33 are X-drop's own (9 and 11 belong to seed_cand and dw)
        if (nredone) atomicAdd(&counters[33], nredone);      // blocks redone in place with the wide window
#ifdef MECAT_XD_STATS
        if (!WIDE) {
            atomicAdd(&counters[16], __builtin_amdgcn_s_memtime() - tk_life);      // wave life, ticks
            for (int i = 0; i < 7; ++i) atomicAdd(&counters[17 + i], xs[i]);         // stage, rows, trace ticks; two-pass rows, window loads, traceback steps, query refills
            atomicAdd(&counters[24], 1ull);
        }
#endif
    }
}

// XdropAligner::go tail (xdrop_gapalign.cpp:396-438): the left half is emitted without its last column
__global__ void xd_stitch(const mhip_aln_job* __restrict__ jobs, const XDir* __restrict__ dres, int n, int min_aln,
                          mhip_aln_result* __restrict__ out, unsigned long long* __restrict__ counters) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    XDir L = dres[2 * i];
    const XDir R = dres[2 * i + 1];
    if (L.columns > 0) { L.columns -= 1; L.qbases -= L.last_q; L.tbases -= L.last_t; L.matches -= L.last_m; }
    mhip_aln_result r;
    r.query_start = jobs[i].qstart - L.qbases;
    r.target_start = jobs[i].sstart - L.tbases;
    r.query_end = jobs[i].qstart + R.qbases;
    r.target_end = jobs[i].sstart + R.tbases;
    r.matches = L.matches + R.matches;
    r.columns = L.columns + R.columns;
    r.blocks = L.blocks + R.blocks;
    r.ok = (r.query_end - r.query_start) >= min_aln;      // :438
    out[i] = r;
    if (r.ok) {
        atomicAdd(&counters[6], (unsigned long long)(r.query_end - r.query_start));
        atomicAdd(&counters[7], 1ull);
    }
}

// ---- the launch.  Which arrangement runs is read from the environment once per call:
struct XdMode {
    bool all_wide;        // MECAT_XD_WIDE=1: every block of every unit through the wide block (cross-check of the ring block, tests)
    bool handover;        // MECAT_XD_HANDOVER=1: units with a block that outgrows the ring go to a second launch (tests compare the two)
    bool order;           // MECAT_XD_ORDER=0: jobs in candidate order, not longest first
    int waves_per_cu;     // MECAT_XW_WAVES: resident ring waves per CU (24)
};
static XdMode xd_mode() {
    auto is = [](const char* name, int v) { const char* s = getenv(name); return s && atoi(s) == v; };
    XdMode m;
    m.all_wide = is("MECAT_XD_WIDE", 1);
    m.handover = is("MECAT_XD_HANDOVER", 1);
    m.order = !is("MECAT_XD_ORDER", 0);
    m.waves_per_cu = getenv("MECAT_XW_WAVES") ? atoi(getenv("MECAT_XW_WAVES")) : 24;
    return m;
}

// Every unit of jobs [0, n) through the ring kernel, in place or (handover) with the units it could not finish listed in d_ovf;
// *nwide = their number.  Waits for the stream.
static int xd_launch_ring(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, bool handover, int waves,
                          XDir* d_dres, unsigned int* d_cur, unsigned int* d_ovf, const unsigned int* d_order, unsigned int* nwide) {
    const int grid = std::min(waves / XW_WAVES, (2 * n + XW_WAVES - 1) / XW_WAVES);
    const size_t launched = (size_t)grid * XW_WAVES;      // both per-wave buffers are sized for the waves this call launches
    uint8_t *d_s, *d_wst = nullptr;
    if (c->scratch("xw_state", XR_STATE_BYTES * launched, (void**)&d_s)) return -1;
    if (!handover && c->scratch("xw_inplace", XW_INPLACE_BYTES * launched, (void**)&d_wst)) return -1;
    LAUNCH(c, "xd_extend_w", xd_extend_w<false>, grid, XW_BLOCK, 0, (const uint32_t*)ref->d_pac, (const mhip_offset_t*)ref->d_offs,
           (const uint32_t*)reads->d_pac, (const mhip_offset_t*)reads->d_offs, (const mhip_aln_job*)d_jobs, n, d_dres, d_s, d_cur,
           d_ovf, (unsigned long long*)c->d_counters, (const unsigned int*)nullptr, 2u * (unsigned)n, d_wst, d_order);
    HIPCHK(hipMemcpyAsync(nwide, d_ovf, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (getenv("MECAT_TRACE")) {
        if (d_wst) {
            unsigned long long redone = 0;
            HIPCHK(hipMemcpy(&redone, (unsigned long long*)c->d_counters + 33, sizeof(redone), hipMemcpyDeviceToHost));
            fprintf(stderr, "[mecat_hip] X-drop: %d units, %llu blocks so far redone in place with the wide window\n", 2 * n, redone);
        } else fprintf(stderr, "[mecat_hip] X-drop: %u of %d units need the wide-window path\n", *nwide, 2 * n);
    }
    return 0;
}

// The wide kernel, one wave per workgroup: the nu units listed in ulist from where they stand, or (ulist == NULL) units [0, nu) from their start
static int xd_launch_wide(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, XDir* d_dres,
                          unsigned int* d_cur, unsigned int* d_ovf, const unsigned int* ulist, unsigned int nu) {
    const int wgrid = (int)std::min(nu, 2048u);
    uint8_t* d_w;
    if (c->scratch("xw_wide", XW_WIDE_BYTES * (size_t)wgrid, (void**)&d_w)) return -1;
    LAUNCH(c, "xd_extend_wide", xd_extend_w<true>, wgrid, 64, 0, (const uint32_t*)ref->d_pac, (const mhip_offset_t*)ref->d_offs,
           (const uint32_t*)reads->d_pac, (const mhip_offset_t*)reads->d_offs, (const mhip_aln_job*)d_jobs, n, d_dres, d_w, d_cur + 2,
           d_ovf + 6 * (size_t)n + 4, (unsigned long long*)c->d_counters, ulist, nu, (uint8_t*)nullptr, (const unsigned int*)nullptr);
    return 0;
}

extern "C" {

int mhip_xalign_candidates_dev(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n,
                               int min_align_size, void* d_out) {
    HIPCHK(hipSetDevice(c->device));
    if (n <= 0) return 0;
    const XdMode mode = xd_mode();
    XDir* d_dres;
    unsigned int *d_cur, *d_ovf;
    if (c->scratch("xa_dres", sizeof(XDir) * 2 * (size_t)n, (void**)&d_dres)) return -1;
    if (c->scratch("xa_cursor", 64, (void**)&d_cur)) return -1;
    if (c->scratch("xa_ovf", sizeof(unsigned int) * (6 * (size_t)n + 8), (void**)&d_ovf)) return -1;      // count + {unit, qidx, tidx} each
    HIPCHK(hipMemsetAsync(d_cur, 0, 16, c->stream));
    unsigned int nwide = 0;
    if (!mode.all_wide) {
        const int waves = c->num_cus * mode.waves_per_cu;
        HIPCHK(hipMemsetAsync(d_ovf, 0, sizeof(unsigned int), c->stream));
        unsigned int* d_order = nullptr;
        if (mode.order && xd_order_jobs(c, ref, reads, d_jobs, n, waves, &d_order)) return -1;
        if (xd_launch_ring(c, ref, reads, d_jobs, n, mode.handover, waves, d_dres, d_cur, d_ovf, d_order, &nwide)) return -1;
    }
    if (nwide > 0 || mode.all_wide) {
        const unsigned int* ulist = mode.all_wide ? nullptr : d_ovf + 1;
        if (xd_launch_wide(c, ref, reads, d_jobs, n, d_dres, d_cur, d_ovf, ulist, mode.all_wide ? 2u * (unsigned)n : nwide)) return -1;
    }
    LAUNCH(c, "xd_stitch", xd_stitch, (n + 255) / 256, 256, 0, (const mhip_aln_job*)d_jobs, (const XDir*)d_dres, n, min_align_size,
           (mhip_aln_result*)d_out, (unsigned long long*)c->d_counters);
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int mhip_xalign_candidates(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const mhip_aln_job* jobs, int n,
                           int min_align_size, mhip_aln_result* out) {
    return aln_jobs_run(c, ref, reads, jobs, n, min_align_size, out, mhip_xalign_candidates_dev);
}

}  // extern "C"
