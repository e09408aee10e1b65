// seed_walk.h — the 1 024-thread workgroup's scan and pipelined bucket walk, shared by seed_filter_wide (seed_chain.hip) and
// seed_strand (seed_strand.hip)
#pragma once

#include "seed_defs.h"

#define FS_THREADS 1024
#define FS_WAVES (FS_THREADS / WAVE)

// block-wide exclusive scan, FS_THREADS threads.  The thread index is an argument (as in fs_walk and fs_block_sum2): seed_strand hands in
// a copy the compiler cannot see through, so that the lane masks and shuffle addresses are made where they are used and not once in
// front of its strand loop, where they would occupy registers through every phase.
__device__ __forceinline__ uint32_t fs_excl_scan(const int tid, uint32_t v, uint32_t* wtot, uint32_t* total) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t n = (uint32_t)__builtin_amdgcn_ds_bpermute(((lane - o) & 63) << 2, (int)incl);
        if (lane >= o) incl += n;
    }
    __syncthreads();
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < FS_WAVES; ++w) {
        const uint32_t x = wtot[w];
        if (w < wave) base += x;
        tot += x;
    }
    *total = tot;
    return base + incl - v;
}

// pipelined walk over the buckets of a strand; f(km, value) per hit.  LPB lanes per bucket, Q buckets per group and stage, D stages
// of bucket data in flight plus one stage of bucket headers (start, size) ahead of them.  The first NP * LPB entries of a bucket are
// loaded by the pipeline (NP pieces of LPB); a longer bucket reads the rest when it is consumed.
// The headers come from `kbs` / `kcn`: the km_* arrays in HBM (seed_filter_wide) or a strand's copy in LDS (seed_strand, 16-bit counts).
template <int LPB, int NP, int Q, int D, bool UNIFORM, typename T, typename C, typename F>
__device__ __forceinline__ void fs_walk(const int tid, const uint32_t* __restrict__ kbs, const C* __restrict__ kcn, const T* __restrict__ arr,
                                        const int K, F f) {
    constexpr int G = FS_THREADS / LPB, STEP = Q * G;
    const int g = tid / LPB;
    const uint32_t sub = (uint32_t)tid % LPB;
    uint32_t hb[Q], hc[Q];                          // headers of stage D (no data requested yet)
    uint32_t sb[D][Q], sc[D][Q], sd[D][Q][NP];      // stages 0 .. D-1: header and data
#define FS_HDR(BASE, BS, CN)                                                      \
    _Pragma("unroll") for (int q = 0; q < Q; ++q) {                               \
        const int km_ = (BASE) + q * G + g;                                       \
        BS[q] = km_ < K ? kbs[km_] : 0u;                                          \
        CN[q] = km_ < K ? (uint32_t)kcn[km_] : 0u;                                \
    }
#define FS_DAT(BS, CN, DD)                                                        \
    _Pragma("unroll") for (int q = 0; q < Q; ++q)                                 \
        _Pragma("unroll") for (int p = 0; p < NP; ++p)                            \
            DD[q][p] = sub + (uint32_t)(p * LPB) < CN[q] ? (uint32_t)arr[BS[q] + (uint32_t)(p * LPB) + sub] : 0u;
#pragma unroll
    for (int d = 0; d < D; ++d) { FS_HDR(d * STEP, sb[d], sc[d]) }
    FS_HDR(D * STEP, hb, hc)
#pragma unroll
    for (int d = 0; d < D; ++d) { FS_DAT(sb[d], sc[d], sd[d]) }
    for (int base = 0; base < K; base += STEP) {
        uint32_t cb[Q], cc[Q], cd[Q][NP];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            cb[q] = sb[0][q]; cc[q] = sc[0][q];
#pragma unroll
            for (int p = 0; p < NP; ++p) cd[q][p] = sd[0][q][p];
        }
#pragma unroll
        for (int d = 0; d + 1 < D; ++d)
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                sb[d][q] = sb[d + 1][q]; sc[d][q] = sc[d + 1][q];
#pragma unroll
                for (int p = 0; p < NP; ++p) sd[d][q][p] = sd[d + 1][q][p];
            }
#pragma unroll
        for (int q = 0; q < Q; ++q) { sb[D - 1][q] = hb[q]; sc[D - 1][q] = hc[q]; }
        FS_DAT(sb[D - 1], sc[D - 1], sd[D - 1])
        FS_HDR(base + (D + 1) * STEP, hb, hc)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int km = base + q * G + g;
            if constexpr (UNIFORM) {            // f(km, value, valid) is called by the whole wave together
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const bool v = sub + (uint32_t)(p * LPB) < cc[q];
                    if (__any(v)) f(km, cd[q][p], v);
                }
                // (what the pipeline did not cover, four pieces per round trip: one by one each piece is a memory latency for the whole wave)
                for (uint32_t r = (uint32_t)(NP * LPB) + sub; __any(r < cc[q]); r += 4 * LPB) {
                    uint32_t tv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) tv[u] = r + (uint32_t)(u * LPB) < cc[q] ? (uint32_t)arr[cb[q] + r + (uint32_t)(u * LPB)] : 0u;
#pragma unroll
                    for (int u = 0; u < 4; ++u) { const bool v = r + (uint32_t)(u * LPB) < cc[q]; if (__any(v)) f(km, tv[u], v); }
                }
            } else {
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    if (sub + (uint32_t)(p * LPB) < cc[q]) f(km, cd[q][p]);
                for (uint32_t r = (uint32_t)(NP * LPB) + sub; r < cc[q]; r += 4 * LPB) {      // (four pieces per round trip, see above)
                    uint32_t tv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) tv[u] = r + (uint32_t)(u * LPB) < cc[q] ? (uint32_t)arr[cb[q] + r + (uint32_t)(u * LPB)] : 0u;
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (r + (uint32_t)(u * LPB) < cc[q]) f(km, tv[u]);
                }
            }
        }
    }
#undef FS_HDR
#undef FS_DAT
}
