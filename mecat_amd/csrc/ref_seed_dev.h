// ref_seed_dev.h — what mecat2ref's kernels share of the seeding stage (ref_seed.hip: candidate lists; ref_rescue.hip: the rescue's
// searches, which need a strand's segment records again): the virtual segment array of a wave (directory + record pool), the seeding
// loop of reference_mapping (mecat2ref/mecat2ref_impl_large.cpp:417-453 with insert_loc :92-130), the DDF test, the pairwise vote and
// find_location's selection (mecat2ref_aux.cpp:6-83), and the host side that sizes and clears the pools.  See ref_seed.hip's head for
// the scheme; everything here is __forceinline__ into its one call site per kernel.
#pragma once

#include <stdlib.h>

#include <algorithm>

#include "common.h"

#define RF_SM 20                     // seeds stored per segment (SM, mecat2ref_defs.h:22)
#define RF_MAXC 100                  // longest list a call may ask for
#define RF_RM 100000                 // the reference's read buffers (RM, mecat2ref_defs.h:16)
#define RF_REC 44                    // shorts of one record: score, loczhi[20], seedno[20], seednum, index (two shorts)
#define R_SCORE 0
#define R_LOC 1
#define R_SEED (1 + RF_SM)
#define R_SEEDNUM (1 + 2 * RF_SM)
#define R_INDEX (2 + 2 * RF_SM)      // int at short offset 42 (byte 84)
#define RF_BLOCK 256
#define RF_POOL 2048                 // records of a wave's pool (176 KB); a read that needs more is redone with a worst-case pool
#define RF_WAVES (RF_BLOCK / WAVE)

template <int NCAND>
struct RefWaveLdsT {
    int tl[64], ts[64], tsc[64];     // find_location's lists (at most 2 * 20 entries) / insert_loc's 21
    mhip_ref_candidate cand[NCAND];  // the read's list (ref_seed) / its rescue candidates (ref_rescue_find)
};
typedef RefWaveLdsT<RF_MAXC> RefWaveLds;

// ---------------------------------------------------------------- host: a launch's directories and pools
struct RfPools {
    short *pool = nullptr, *iscore = nullptr;
    uint32_t* dir = nullptr;
    int *ilist = nullptr, *slotseg = nullptr, *hw = nullptr;
    unsigned int* cur = nullptr;     // 16 words: [0] the read cursor, [4] most records a wave initialised, [5] reads given up
    size_t waves = 0, free_b = 0;
    unsigned grid = 0;
    int pcap = 0, nseg = 0;
};
inline size_t rf_rec_bytes() { return RF_REC * sizeof(short) + sizeof(int) + sizeof(short) + sizeof(int); }

// One directory + record pool per resident wave, 12 waves per CU (the seeding kernel's registers allow 3 per SIMD), fewer when they would
// take more than half of the free memory.  MECAT_REF_POOL overrides the pool's records (the test of the second launch makes it small).
// Directories, hw and the cursor words are cleared on the context's stream.
inline int rf_pools_first(mhip_ctx* c, int nseg, int n, RfPools* P) {
    const char* pe = getenv("MECAT_REF_POOL");
    const int pcap = std::min(nseg + 1, std::max(8, pe && atoi(pe) > 0 ? atoi(pe) : RF_POOL));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t per_wave = (size_t)pcap * rf_rec_bytes() + (size_t)(nseg + 8) * sizeof(uint32_t);
    const size_t max_waves = (size_t)c->num_cus * 12;
    size_t waves = std::min<size_t>(max_waves, std::max<size_t>(1, free_b / 2 / per_wave));
    waves = std::min<size_t>(waves, (size_t)n);
    const unsigned grid = (unsigned)((waves + RF_WAVES - 1) / RF_WAVES);
    waves = (size_t)grid * RF_WAVES;
    if (c->scratch("rf_pool", sizeof(short) * waves * (size_t)pcap * RF_REC, (void**)&P->pool)) return -1;
    if (c->scratch("rf_dir", sizeof(uint32_t) * waves * (size_t)(nseg + 8), (void**)&P->dir)) return -1;
    if (c->scratch("rf_hw", sizeof(int) * waves, (void**)&P->hw)) return -1;
    if (c->scratch("rf_ilist", sizeof(int) * waves * (size_t)pcap, (void**)&P->ilist)) return -1;
    if (c->scratch("rf_iscore", sizeof(short) * waves * (size_t)pcap, (void**)&P->iscore)) return -1;
    if (c->scratch("rf_slotseg", sizeof(int) * waves * (size_t)pcap, (void**)&P->slotseg)) return -1;
    if (c->scratch("rf_cursor", 64, (void**)&P->cur)) return -1;
    HIPCHK(hipMemsetAsync(P->dir, 0, sizeof(uint32_t) * waves * (size_t)(nseg + 8), c->stream));
    HIPCHK(hipMemsetAsync(P->hw, 0, sizeof(int) * waves, c->stream));        // (the pools count as uninitialised: records are set up as they are handed out)
    HIPCHK(hipMemsetAsync(P->cur, 0, 64, c->stream));
    P->waves = waves; P->grid = grid; P->pcap = pcap; P->nseg = nseg; P->free_b = free_b;
    return 0;
}

// the launch for the reads that ran out of records, with pools that cannot (one record per segment): few waves, their own pool buffers;
// directories (all zero again) and the cursor words are the first launch's
inline int rf_pools_full(mhip_ctx* c, const RfPools& first, size_t nredo, const char* who, RfPools* P) {
    const int full = first.nseg + 1;
    size_t w2 = std::min<size_t>(std::min<size_t>(first.waves, nredo), std::max<size_t>(1, first.free_b / 4 / ((size_t)full * rf_rec_bytes())));
    const unsigned grid2 = (unsigned)((w2 + RF_WAVES - 1) / RF_WAVES);
    w2 = (size_t)grid2 * RF_WAVES;
    if (w2 > first.waves) { mhip_set_error("%s: no room for the worst-case pools of %zu reads", who, nredo); return -1; }
    *P = first;
    if (c->scratch("rf_pool_full", sizeof(short) * w2 * (size_t)full * RF_REC, (void**)&P->pool)) return -1;
    if (c->scratch("rf_ilist_full", sizeof(int) * w2 * (size_t)full, (void**)&P->ilist)) return -1;
    if (c->scratch("rf_iscore_full", sizeof(short) * w2 * (size_t)full, (void**)&P->iscore)) return -1;
    if (c->scratch("rf_slotseg_full", sizeof(int) * w2 * (size_t)full, (void**)&P->slotseg)) return -1;
    if (c->scratch("rf_hw_full", sizeof(int) * w2, (void**)&P->hw)) return -1;
    HIPCHK(hipMemsetAsync(P->hw, 0, sizeof(int) * w2, c->stream));
    HIPCHK(hipMemsetAsync(P->cur, 0, 64, c->stream));
    P->waves = w2; P->grid = grid2; P->pcap = full;
    return 0;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- device
typedef volatile short vshort;       // the segment records are re-read after other lanes wrote them: no L1 / register caching

__device__ __forceinline__ int rf_index(vshort* r) { return (int)(uint16_t)r[R_INDEX] | ((int)r[R_INDEX + 1] << 16); }
__device__ __forceinline__ void rf_set_index(vshort* r, int v) { r[R_INDEX] = (short)(v & 0xffff); r[R_INDEX + 1] = (short)(v >> 16); }

__device__ __forceinline__ void rf_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the DDF test of find_location (mecat2ref_aux.cpp:10: fabs(int / (int * float) - 1) < double, all f32 up to the comparison) and of
// insert_loc (mecat2ref_impl_large.cpp:106: `- 1.0`, so the subtraction is f64)
template <bool SUB_F64>
__device__ __forceinline__ bool rf_ddf(int dloc, int dseed, float bc, double cutoff) {
    const float q = (float)dloc / ((float)dseed * bc);
    if (SUB_F64) return fabs((double)q - 1.0) < cutoff;
    return (double)fabsf(q - 1.0f) < cutoff;
}

// the pairwise vote over S.tl / S.ts [0, n), n <= 64: entry i per lane, its j > i in order; votes into S.tsc (zeroed by the caller).
// dist_cap: find_location's `t_loc[j] - t_loc[i] < read_len`; insert_loc has no such term.
template <bool SUB_F64, class LDS>
__device__ __forceinline__ void rf_vote(LDS& S, int n, int lane, float bc, double cutoff, int dist_cap) {
    if (lane < n - 1) {
        const int li = S.tl[lane], si = S.ts[lane];
        int mine = 0;
        for (int j = lane + 1; j < n; ++j) {
            const int dl = S.tl[j] - li, ds = S.ts[j] - si;
            if (ds > 0 && dl > 0 && dl < dist_cap && rf_ddf<SUB_F64>(dl, ds, bc, cutoff)) {
                ++mine;
                atomicAdd(&S.tsc[j], 1);
            }
        }
        if (mine) atomicAdd(&S.tsc[lane], mine);
    }
    __builtin_amdgcn_wave_barrier();
}

// find_location's choice behind the vote over S.tl / S.ts / S.tsc [0, nl) (mecat2ref_aux.cpp:24-82); false = no location
template <class LDS>
__device__ __forceinline__ bool rf_select(const LDS& S, int nl, int L, float bcf, double cutoff, int& loc0, int& loc1, int& rep_loc) {
    int flag = 0;
    loc0 = loc1 = rep_loc = 0;
    int maxval = 0, maxi = 0, rep = 0;
    for (int j = 0; j < nl; ++j) {
        const int v = S.tsc[j];
        if (maxval < v) { maxval = v; maxi = j; rep = 0; }
        else if (maxval == v) ++rep;
    }
    if (maxval >= 5 && rep == maxval) { flag = 1; loc0 = S.tl[maxi]; loc1 = S.ts[maxi]; rep_loc = maxi; }
    else if (maxval >= 5) {
        // the entries that agree with the best one, in index order (before it, itself, after it): each is taken as the start
        // point while none is held — "none" is `loc[0] == 0` in the reference (mecat2ref_aux.cpp:40-79)
        flag = 1;
        const int lm = S.tl[maxi], sm = S.ts[maxi];
        for (int j = 0; j < maxi; ++j) {
            const int lj = S.tl[j], sj = S.ts[j];
            if (sm - sj > 0 && lm - lj > 0 && lm - lj < L && rf_ddf<false>(lm - lj, sm - sj, bcf, cutoff) && loc0 == 0) { loc0 = lj; loc1 = sj; rep_loc = j; }
        }
        if (loc0 == 0) { loc0 = lm; loc1 = sm; rep_loc = maxi; }
        for (int j = maxi + 1; j < nl; ++j) {
            const int lj = S.tl[j], sj = S.ts[j];
            if (sj - sm > 0 && lj - lm > 0 && lj - lm <= L && rf_ddf<false>(lj - lm, sj - sm, bcf, cutoff) && loc0 == 0) { loc0 = lj; loc1 = sj; rep_loc = j; }
        }
    }
    return flag != 0;
}

// a wave's virtual segment array: the directory (one record number per segment, 0 = untouched) and the pool the records come from
struct RfWave {
    vshort* pool;                    // pcap records; record 0 = the untouched record
    volatile uint32_t* dir;
    int* ilist;
    volatile short* iscore;
    volatile int* slotseg;
    int pcap;
    int hw;                          // records [0, hw) of the pool have been initialised and are in the untouched state
    int nslots;                      // records handed out to the strand in hand: [1, nslots)

    __device__ __forceinline__ vshort* rec(int seg) const { return pool + (size_t)dir[seg] * RF_REC; }
    __device__ __forceinline__ void init_records(int from, int to, int lane) {
        for (int r = from; r < to; ++r) {
            vshort* q = pool + (size_t)r * RF_REC;
            if (lane < RF_REC - 2) q[lane] = 0;
            if (lane == 0) rf_set_index(q, -1);
        }
    }
    __device__ __forceinline__ void bind(size_t gw, short* pool_all, uint32_t* dir_all, int* hw_all, int* ilist_all, short* iscore_all, int* slotseg_all,
                                         int nseg, int pcap_, int lane) {
        pool = pool_all + gw * (size_t)pcap_ * RF_REC;
        dir = dir_all + gw * (size_t)(nseg + 8);
        ilist = ilist_all + gw * (size_t)pcap_;
        iscore = iscore_all + gw * (size_t)pcap_;
        slotseg = slotseg_all + gw * (size_t)pcap_;
        pcap = pcap_;
        hw = hw_all[gw];
        if (hw == 0) { init_records(0, 1, lane); hw = 1; }
        nslots = 1;
        rf_sync();
    }
    // the strand is done (or given up): its records go back to the untouched state (one contiguous stretch of the pool) and their
    // segments' directory entries to 0
    __device__ __forceinline__ void release(int lane) {
        volatile uint32_t* w = (volatile uint32_t*)(pool + RF_REC);         // (RF_REC shorts = 22 words per record)
        const int nw = (nslots - 1) * (RF_REC / 2);
        for (int j = lane; j < nw; j += 64) w[j] = (j % (RF_REC / 2)) == (RF_REC / 2 - 1) ? 0xffffffffu : 0u;
        for (int sl = 1 + lane; sl < nslots; sl += 64) dir[slotseg[sl]] = 0u;
        nslots = 1;
        rf_sync();
    }
};

// ---- seeding (:417-453) of one strand of the read at qoff (L letters, K k-mers at stride bcq) into W's segments of Z positions.
// Bucket bounds two steps ahead and first positions one step ahead, as in asm_seed.hip.  `touched` counts the segments whose first seed
// arrived (their order and sums are in W.ilist / W.iscore).  false: the read needs more records than the pool has.
template <class LDS>
__device__ __forceinline__ bool rf_seed_strand(RfWave& W, LDS& S, const uint32_t* __restrict__ starts, const int32_t* __restrict__ offsets,
                                               const uint32_t* __restrict__ qpac, const uint32_t* __restrict__ qnpac, int64_t qoff, int L, int K, int bcq,
                                               float bcf, int Z, int strand, double cutoff, int lane, int& touched) {
    const unsigned long long below = (1ull << lane) - 1ull;
    bool ovf = false;
    auto bounds = [&](int k, uint32_t& s0, uint32_t& s1) {
        s0 = s1 = 0;
        if (k >= K) return;
        const int64_t kpos = !strand ? qoff + (int64_t)k * bcq : qoff + L - MHIP_KMER_SIZE - (int64_t)k * bcq;
        // a k-mer with a letter other than upper-case A, C, G, T is not looked up (atcttrans gives 4, :44-51, :79-83)
        if (qnpac && pac_kmer(qnpac, kpos) != 0u) return;
        const uint32_t id = !strand ? pac_kmer(qpac, kpos) : kmer_revcomp(pac_kmer(qpac, kpos));
        s0 = starts[id];
        s1 = starts[id + 1];
    };
    uint32_t s0, s1, n0, n1;
    bounds(0, s0, s1);
    bounds(1, n0, n1);
    int pfirst = s0 + (uint32_t)lane < s1 ? offsets[s0 + (uint32_t)lane] : 0;
    for (int k = 0; k < K; ++k) {
        const int pnext = n0 + (uint32_t)lane < n1 ? offsets[n0 + (uint32_t)lane] : 0;
        uint32_t m0, m1;
        bounds(k + 2, m0, m1);
        int carry_seg = -1;
        for (uint32_t base = s0; base < s1; base += 64) {
            const uint32_t e = base + (uint32_t)lane;
            const bool valid = e < s1;
            const int p = valid ? (base == s0 ? pfirst : offsets[e]) + 1 : 0;          // 1-based k-mer start (i + 2 - seed_len, :265)
            const int seg = valid ? p / Z : -2, off = p % Z;
            int seg_prev = __shfl_up(seg, 1);
            if (lane == 0) seg_prev = carry_seg;
            carry_seg = __shfl(seg, 63);
            const bool head = valid && seg != seg_prev;        // the first hit of this k-mer in its segment
            bool ev = false;
            int newscore = 0;
            // a segment's first hit takes the next record of the pool
            const bool fresh_rec = head && W.dir[seg] == 0u;
            const unsigned long long fm = __ballot(fresh_rec);
            if (fm && W.nslots + (int)__popcll(fm) > W.pcap) { ovf = true; break; }
            if (fm) {
                const int nnew = (int)__popcll(fm);
                if (W.nslots + nnew > W.hw) {
                    W.init_records(W.hw, W.nslots + nnew, lane);
                    W.hw = W.nslots + nnew;
                    rf_sync();
                }
                if (fresh_rec) {
                    const int sl = W.nslots + (int)__popcll(fm & below);
                    W.dir[seg] = (uint32_t)sl;
                    W.slotseg[sl] = seg;
                }
                W.nslots += nnew;
            }
            if (head) {
                vshort* r = W.rec(seg);
                const int sc = r[R_SCORE], sn = r[R_SEEDNUM];
                ev = sc == 0 || sn < k + 1;                    // :429
                if (ev) {
                    newscore = sc + 1;
                    r[R_SCORE] = (short)newscore;
                    if (newscore <= RF_SM) { r[R_LOC + newscore - 1] = (short)off; r[R_SEED + newscore - 1] = (short)(k + 1); }
                }
                r[R_SEEDNUM] = (short)(k + 1);
            }
            // insert_loc (:92-130) for the segments that are past 20 seeds, one after the other, the wave voting over the 21
            unsigned long long need = __ballot(ev && newscore > RF_SM);
            while (need) {
                const int src = __ffsll((long long)need) - 1;
                need &= need - 1;
                rf_sync();
                vshort* r = W.rec(__shfl(seg, src));
                const int noff = __shfl(off, src);
                if (lane < RF_SM) { S.tl[lane] = r[R_LOC + lane]; S.ts[lane] = r[R_SEED + lane]; }
                if (lane == RF_SM) { S.tl[lane] = noff; S.ts[lane] = k + 1; }
                S.tsc[lane] = 0;
                __builtin_amdgcn_wave_barrier();
                rf_vote<true>(S, RF_SM + 1, lane, bcf, cutoff, 0x7fffffff);
                int minval = 10000, mini = -1;                 // (the first entry with the fewest votes)
                for (int j = 0; j <= RF_SM; ++j) {
                    const int v = S.tsc[j];
                    if (minval > v) { minval = v; mini = j; }
                }
                if (minval == RF_SM) {
                    if (lane == 0) { r[R_LOC + RF_SM - 1] = (short)noff; r[R_SEED + RF_SM - 1] = (short)(k + 1); }
                } else if (minval < RF_SM && mini < RF_SM) {
                    if (lane >= mini && lane < RF_SM) { r[R_LOC + lane] = (short)S.tl[lane + 1]; r[R_SEED + lane] = (short)S.ts[lane + 1]; }
                    if (lane == src) { --newscore; r[R_SCORE] = (short)newscore; }
                }
                __builtin_amdgcn_wave_barrier();
            }
            rf_sync();
            int idx = 0;
            if (ev) idx = rf_index(W.rec(seg));
            const unsigned long long fresh = __ballot(ev && idx == -1);
            if (ev) {
                const int sk = seg > 0 ? newscore + (int)W.rec(seg - 1)[R_SCORE] : newscore;      // :438-439
                if (idx == -1) {
                    const int t = touched + (int)__popcll(fresh & below);
                    W.ilist[t] = seg;
                    W.iscore[t] = (short)sk;
                    rf_set_index(W.rec(seg), t);
                } else W.iscore[idx] = (short)sk;
            }
            touched += (int)__popcll(fresh);
            rf_sync();
        }
        if (ovf) break;
        s0 = n0; s1 = n1; pfirst = pnext;
        n0 = m0; n1 = m1;
    }
    return !ovf;
}
#endif
