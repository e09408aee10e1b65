// xd_block_wide.h — the WIDE block of the X-drop aligner: the row formulation of xd_block_ring.h in its plain form, for the blocks
// whose window outgrows the ring (low-complexity sequence keeps hundreds of cells within X of the best score).  Scores indexed by b,
// one script BYTE per cell in rows of XW_WSTRIDE bytes (any window fits), every row's first column in rstart[], and a traceback that
// reads byte by byte through an LDS window over the rows.  Slower per row than the ring and rare; also the ring's cross-check
// (MECAT_XD_WIDE=1 runs every block of every unit through it).  Included by xalign.hip and, with
// a view and a column sink of its own (xd_defs.h: XNoSink), by ref_xextend.hip.
#pragma once
#include "xd_defs.h"

struct XwWide {
    int2 HF[XW_WIDE_HF];                                 // (H, F) of cell b
    uint8_t Qb[X_MAXN + 8], Tb[X_MAXN + 72];             // Tb[b + 1] = target base b (one pad in front, 64 behind for idle lanes)
    int16_t rstart[X_MAXN + 2];                          // first column of every row's script bytes
    uint32_t win[XW_WIN / 4];
};
static_assert(sizeof(XwWide) <= XW_INPLACE_STATE, "the in-place wide state holds one XwWide");

// S: the wave's state, in LDS (xd_extend_w<true>) or in global memory (a ring wave's in-place redo); st: its XW_WIDE_BYTES of script rows
template <class View = XView, class Sink = XNoSink>
__device__ inline void xdrop_block_wide(XwWide& S, const View& q, int qidx, int M, const View& t, int tidx, int N, uint8_t* __restrict__ st,
                                        XBlockOut& o, const Sink& sink = Sink()) {
    auto slot = [&](int b) -> int { return min(b, XW_WIDE_HF - 1); };      // (idle lanes read a valid slot)
    auto ldHF = [&](int b, bool in) -> int2 {
        int2 v = S.HF[slot(b)];
        asm volatile("" : "+v"(v.x), "+v"(v.y));          // every lane loads (the slot is always valid): no exec round trip
        return in ? v : make_int2(X_MIN_SCORE, X_MIN_SCORE);
    };
    auto stHF = [&](int b, int h, int f) { S.HF[slot(b)] = make_int2(h, f); };
    xblock_clear(o);
    if (M <= 0 || N <= 0) return;
    const int lane = lane_id();
    const int X = 30;
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < M; i += 64) S.Qb[i] = (uint8_t)xv_at(q, qidx + i);
    for (int i = lane; i < N; i += 64) S.Tb[i + 1] = (uint8_t)xv_at(t, tidx + i);
    // row 0 (xdrop_gapalign.cpp:45-57): cells 1.. hold -1, -2, ... while >= -X
    const int n_init = min(N, X);
    if (lane == 0) S.rstart[0] = 0;
    if (lane <= n_init) { stHF(lane, -lane, -lane - 1); if (lane) st[lane] = XS_GAP_IN_A; }
    int b_size = n_init + 1, best = 0, first_b = 0, ae = 0, be = 0;      // b_size == N + 1 when N <= X, as in the reference
    __builtin_amdgcn_wave_barrier();
    for (int a = 1; a <= M; ++a) {
        const int AC = S.Qb[a - 1];
        const int f0 = first_b, n0 = b_size;
        o.cells += n0 - f0;
        o.rows = a;
        uint8_t* srow = st + (size_t)a * XW_WSTRIDE;
        int runP = XW_NEG, bb = best, rowarg = -1, firstkept = -1, lastkept = -1, lastkeptH = 0;
        int prevHp = 0;
        auto pass = [&](const int c0) __attribute__((always_inline)) {
            const int b = c0 + lane;
            const bool in = b < n0;
            const int2 hf = ldHF(b, in);
            const int Hp = hf.x, Fp = hf.y;
            const int left = xw_shr1(Hp, prevHp);
            const bool mt = AC == (int)S.Tb[b];                         // target base b - 1
            const int diag = b == f0 ? X_MIN_SCORE : left + (mt ? 1 : -1);
            const int Mv = max(diag, Fp);
            const int incl = xw_scan_max(in ? Mv + b : XW_NEG);
            const int pex = max(xw_shr1(incl, XW_NEG), runP);         // max over all earlier cells of the row of M_j + j
            const int Ec = (b == f0) ? X_MIN_SCORE : pex - b;
            const int Hc = max(Mv, Ec);
            // best so far before cell b = max(bb, max_{j<b} H_j).  No scan needed: a row's scores exceed the best of the rows before
            // by at most the match reward (every H derives from the previous row, at most +1), so all cells above bb hold the same
            // value and only the position of the first one matters.
            const unsigned long long ex = __builtin_amdgcn_ballot_w64(in && Hc > bb);
            int j1 = 64, nb = bb;
            if (ex) { j1 = __ffsll((long long)ex) - 1; nb = __builtin_amdgcn_readlane(Hc, j1); }
            const int bbefore = lane > j1 ? nb : bb;
            const bool kept = in && !(bbefore - Hc > X);
            const unsigned long long km = __builtin_amdgcn_ballot_w64(kept);
            // op bits: SUB unless the column gap, then the row gap, is strictly better (:99-107)
            int sc = diag, script = XS_SUB;
            if (sc < Fp) { script = XS_GAP_IN_B; sc = Fp; }
            const unsigned long long lower = km & ((1ull << lane) - 1ull);
            const int jsrc = lower ? 63 - __clzll((long long)lower) : 0;
            const int Hj = __shfl(Hc, jsrc);
            // a dropped cell compares with the row gap as the sequential row carries it: H of the nearest kept cell to the left - 1
            const int et = lower ? Hj - 1 : (lastkept >= 0 ? lastkeptH - 1 : X_MIN_SCORE);
            if (sc < (kept ? Ec : et)) script = XS_GAP_IN_A;
            if (kept && Fp >= Hc) script += XS_EXT_A;
            if (kept && Ec >= Hc) script += XS_EXT_B;
            // kept: (H, F') with F' = max(F - 1, H - 1) = H - 1 (H >= F); dropped between kept cells: H = MIN, F stays; a leading
            // dropped cell only moves first_b.  One predicated store.
            if (kept || (in && (lower || firstkept >= 0))) stHF(b, kept ? Hc : X_MIN_SCORE, kept ? Hc - 1 : Fp);
            srow[b - f0] = (uint8_t)(script | (mt ? XS_MATCH : 0));          // lanes past the window write bytes nobody reads
            // carries
            runP = max(runP, __builtin_amdgcn_readlane(incl, 63));
            if (ex && rowarg < 0) rowarg = c0 + j1;
            bb = nb;
            if (km) {
                if (firstkept < 0) firstkept = c0 + __ffsll((long long)km) - 1;
                const int lk = 63 - __clzll((long long)km);
                lastkept = c0 + lk;
                lastkeptH = __builtin_amdgcn_readlane(Hc, lk);
            }
            prevHp = __builtin_amdgcn_readlane(Hp, 63);
        };
        // two in three rows fit one pass: with the carries still at their initial constants the compiler drops their bookkeeping
        if (n0 - f0 <= 64) pass(f0);
        else for (int c0 = f0; c0 < n0; c0 += 64) pass(c0);
        if (bb > best) { best = bb; ae = a; be = rowarg; }
        if (firstkept < 0) { first_b = n0; break; }
        first_b = firstkept;
        if (lane == 0) S.rstart[a] = (int16_t)f0;        // the row's first column
        // The window ends after the last kept cell; if that is the row's last cell, the row gap keeps it open while it stays
        // within X of the best (:139-147; H >= E at a kept cell), and a closing (MIN, MIN) cell follows unless the block ends.
        // (b_size is N + 1 in a block with N <= X, where row 0 ran off the end: nothing is appended then.)
        {
            const bool ext = lastkept >= n0 - 1;
            const int e_end = lastkeptH - 1;
            const int bsz0 = ext ? n0 : lastkept + 1;
            const int cnt = max(min(ext ? e_end - (best - X) + 1 : 0, N - bsz0), 0);
            const int sent = bsz0 + cnt < N ? 1 : 0;
            const int bnew = bsz0 + lane;
            const bool tail = lane < cnt;
            if (lane < cnt + sent) stHF(bnew, tail ? e_end - lane : X_MIN_SCORE, tail ? e_end - lane - 1 : X_MIN_SCORE);
            if (tail && bnew - f0 < XW_WSTRIDE - 2) srow[bnew - f0] = XS_GAP_IN_A;
            b_size = bsz0 + cnt + sent;
        }
        __builtin_amdgcn_wave_barrier();
    }
    o.ae = ae; o.be = be;
    // ---- traceback (:165-210) fused with script_to_aligned_string + trim_mismatch_end
    __threadfence();
    __builtin_amdgcn_wave_barrier();
    // window reload: the bytes were written by this wave, so they are read past the L1 (agent scope) — all XW_WIN / 256 loads of a
    // lane in flight at once (volatile loads would serialise one memory round trip each)
    auto load_window = [&](int word0) {
        constexpr int NW = XW_WIN / 4 / 64;
        uint32_t v[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) v[j] = __hip_atomic_load((const uint32_t*)st + word0 + lane + 64 * j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int j = 0; j < NW; ++j) S.win[lane + 64 * j] = v[j];
    };
    int wbase = 1 << 30;                                 // first scratch byte in the LDS window; nothing loaded yet
    auto row_start = [&](int a) -> int { return __builtin_amdgcn_readfirstlane((int)S.rstart[a]); };
    auto wide_byte = [&](int a, int b, int rs) -> int {
        const int idx = a * XW_WSTRIDE + (b - rs);
        if (idx < wbase || idx >= wbase + XW_WIN) {
            __builtin_amdgcn_wave_barrier();
            wbase = max(((idx + 4) & ~3) - XW_WIN, 0);
            load_window(wbase / 4);
            __builtin_amdgcn_wave_barrier();
        }
        return __builtin_amdgcn_readfirstlane((int)((const uint8_t*)S.win)[idx - wbase]);
    };
    int a_index = ae, b_index = be;
    // One step = one byte: the op is the previous one while its extension bit is set in this byte, else the byte's own
    // (bit 4 continues GAP_IN_A, bit 6 GAP_IN_B; bit 5 is never set and stands in for "after a substitution").
    int st_op = XS_SUB;
    XTail T;
    int crs, nrs = 0;                                    // first column of the current row, of the one before
    crs = row_start(a_index);
    if (a_index > 0) nrs = row_start(a_index - 1);
    while (a_index > 0 || b_index > 0) {
        const int byte = wide_byte(a_index, b_index, crs);
        const int sh = 4 + (st_op & 1) + ((st_op >> 2) << 1);
        const int op = ((byte >> sh) & 1) ? st_op : (byte & XS_OP_MASK);
        st_op = op;
        const int cq = op != XS_GAP_IN_A, ct = op != XS_GAP_IN_B;
        const int cm = cq & ct & (byte >> 7);
        a_index -= cq;
        b_index -= ct;
        if (!(cq & ct)) sink.gap(T.n, cq ? 2 : 1);
        T.step(cq, ct, cm, a_index, b_index);
        if (cq) {
            crs = nrs;
            if (a_index > 0) nrs = row_start(a_index - 1);
        }
    }
    T.finish(ae, be, o);
}
