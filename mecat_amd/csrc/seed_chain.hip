// seed_chain.hip — the kernel chain of the seeding stage and its launchers (seed.hip describes the stage and which strand takes the chain):
//   seed_probe, seed_filter | seed_filter_wide, seed_scan, seed_emit, seed_sort_pass, seed_build
#include <algorithm>

#include "scan.h"
#include "seed_defs.h"
#include "seed_replay.h"
#include "seed_walk.h"

#define GATE_LDS 2048                // gated segments whose first-touch times fit the LDS stage of seed_build

// block-wide exclusive scan of one value per thread (SEED_BLOCK threads); returns the exclusive prefix, total in *total
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wtot /*[SEED_WAVES]*/, uint32_t* total) {
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t n = __shfl_up(incl, o);
        if (lane_id() >= o) incl += n;
    }
    __syncthreads();   // protect wtot from the previous use
    if (lane_id() == 63) wtot[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SEED_WAVES; ++w) {
        if (w < (int)(threadIdx.x >> 6)) base += wtot[w];
        tot += wtot[w];
    }
    *total = tot;
    return base + incl - v;
}

// ------------------------------------------------------------------------------------------------ probe
// `recs` (index.hip: idx_cut_records) replaces starts[] when reference and query volume are the same one (a diagonal grid cell):
// the bucket of a query k-mer is cut at the first of seven fixed positions behind the read's own copy + 5 segments.  What lies
// behind belongs to reads with higher ids: get_candidates drops their candidates at `sid > read_id` (pw_impl.cpp:370) before it writes
// anything, the sweeps of a kept candidate stay within 3 segments of its subject read's end (num2 <= send - loc_list, :399-403,
// 424-438), index_score looks at the left neighbour only (:270-280) — so those hits cannot reach the output, and half of the
// bucket walk of a diagonal cell is not done.  counters[1] still counts every bucket hit (the H of SURVEY.md §8d).
__global__ __launch_bounds__(SEED_BLOCK) void seed_probe(const uint32_t* __restrict__ pac, const mhip_offset_t* __restrict__ roffs,
                                                         ReadSel sel, int ib, const uint32_t* __restrict__ starts, SeedArrays A,
                                                         unsigned long long* __restrict__ counters, const uint4* __restrict__ recs, int cut_step,
                                                         int tally) {
    __shared__ uint32_t wtot[SEED_WAVES];
    const int s = blockIdx.x;
    const int rid = sel_rid(sel, ib + (s >> 1));
    const bool rev = s & 1;
    const int off = roffs[rid].offset, L = roffs[rid].size;
    const int K = kmers_of(L);
    const uint32_t kb = A.km_base[s];
    // byte of the record's y:z that holds the bucket length for this read: cut t = ceil((end of the read + 5 segments) / step)
    int cut_byte = 7;
    if (recs) {
        const long long need = (long long)off + L + 1 + 5 * ZV;
        const long long t = (need + cut_step - 1) / cut_step;
        if (t <= 7) cut_byte = (int)t - 1;
    }
    uint32_t run = 0, run_all = 0;
    for (int t0 = 0; t0 < K; t0 += SEED_BLOCK) {
        int km = t0 + threadIdx.x;
        uint32_t cnt = 0, all = 0, bs = 0;
        if (km < K) {
            uint32_t id;
            if (!rev) id = pac_kmer(pac, (int64_t)off + (int64_t)km * BC);
            else id = kmer_revcomp(pac_kmer(pac, (int64_t)off + L - MHIP_KMER_SIZE - (int64_t)km * BC));
            if (recs) {
                const uint4 r = recs[id];
                const unsigned long long yz = ((unsigned long long)r.z << 32) | r.y;
                bs = r.x;
                all = r.z >> 24;
                cnt = (uint32_t)(yz >> (8 * cut_byte)) & 0xFFu;
            } else {
                bs = starts[id];
                all = cnt = starts[id + 1] - bs;
            }
        }
        uint32_t tot;
        if (recs) {
            (void)block_excl_scan(cnt | (all << 16), wtot, &tot);      // both sums in one scan: <= 256 x 255 each
            run += tot & 0xFFFFu;
            run_all += tot >> 16;
        } else {
            (void)block_excl_scan(cnt, wtot, &tot);
            run += tot;
            run_all += tot;
        }
        if (km < K) {
            A.km_bstart[kb + km] = bs;
            A.km_cnt[kb + km] = cnt;
        }
    }
    if (threadIdx.x == 0) {
        A.strand_hits_all[s] = run;
        if (tally) {                // (0: seed_strand has counted these lookups already and only the km_* arrays are wanted, see seed_batch)
            atomicAdd(&counters[0], (unsigned long long)K);
            atomicAdd(&counters[1], (unsigned long long)run_all);
            if (recs) atomicAdd(&counters[15], (unsigned long long)run);      // debug slot 15: bucket hits walked with the cuts on
        }
    }
}

// exclusive scan of strand_hits[ns] -> hit_base[ns + 1] (single block, sequential over tiles)
__global__ __launch_bounds__(1024) void seed_scan(const uint32_t* __restrict__ hits, int ns, uint64_t* __restrict__ base) {
    const uint64_t total = scan_array_1024<uint64_t>(ns, 0, [&](long long i) { return hits[i]; }, [&](long long i, uint64_t p) { base[i] = p; });
    if (threadIdx.x == 0) base[ns] = total;
}

// ------------------------------------------------------------------------------------------------ hit iteration
// 16 lanes per query k-mer: a bucket (<= 128 ascending positions, ~22 on average) is read in 64-byte pieces, lane `sub`
// takes entries sub, sub + 16, ...  `f(km, r, pos, valid)` is called by all 16 lanes of the group together (group-uniform
// control flow), so it may use the group's 16 bits of a wave ballot.
// Four buckets per group are in flight at once (their (start, size) and first two 64-byte pieces are loaded before any is
// consumed): the walk is a gather of ~88-byte runs, so throughput comes from outstanding loads, not from arithmetic.
// `begin(slot, km)`, `f(slot, km, r, pos, valid)`, `end(slot, km)`; slot 0..3 is a compile-time index for per-bucket state.
template <typename T, typename B, typename F, typename E>
__device__ __forceinline__ void for_each_hit16(const SeedArrays& A, const T* __restrict__ offsets, const uint32_t kb, const int K,
                                               B begin, F f, E end) {
    const int g = threadIdx.x >> 4, sub = threadIdx.x & 15;
    constexpr int G = SEED_BLOCK / 16;
    for (int km0 = g; km0 < K; km0 += 4 * G) {
        uint32_t bs[4], cnt[4], p0[4], p1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int km = km0 + q * G;
            bs[q] = km < K ? A.km_bstart[kb + km] : 0u;
            cnt[q] = km < K ? A.km_cnt[kb + km] : 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            p0[q] = (uint32_t)sub < cnt[q] ? (uint32_t)offsets[bs[q] + sub] : 0u;
            p1[q] = (uint32_t)sub + 16u < cnt[q] ? (uint32_t)offsets[bs[q] + 16 + sub] : 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int km = km0 + q * G;
            if (km < K) {
                begin(q, km);
                if (cnt[q] > 0) f(q, km, (uint32_t)sub, p0[q], (uint32_t)sub < cnt[q]);
                if (cnt[q] > 16) f(q, km, (uint32_t)sub + 16u, p1[q], (uint32_t)sub + 16u < cnt[q]);
                for (uint32_t r0 = 32; r0 < cnt[q]; r0 += 16) {
                    const uint32_t r = r0 + sub;
                    const bool valid = r < cnt[q];
                    f(q, km, r, valid ? (uint32_t)offsets[bs[q] + r] : 0u, valid);
                }
                end(q, km);
            }
        }
    }
}
__device__ __forceinline__ uint32_t group_bits(unsigned long long ballot) { return (uint32_t)(ballot >> (threadIdx.x & 48)) & 0xFFFFu; }

__device__ __forceinline__ bool rel_test(const uint32_t* rel, uint32_t seg) {
    const uint32_t e = seg & (FLT_M - 1);
    return (rel[e >> 5] >> (e & 31u)) & 1u;
}
// the same with the bitmap's geometry as data (seed_emit: bitmaps of seed_filter and of seed_filter_wide)
__device__ __forceinline__ bool rel_test(const uint32_t* rel, uint32_t seg, uint32_t mask, uint32_t shift) {
    const uint32_t e = (seg & mask) >> shift;
    return (rel[e >> 5] >> (e & 31u)) & 1u;
}

// ------------------------------------------------------------------------------------------------ relevance filter
// Most bucket hits are random 13-mer matches that land alone in their 2 kb segment and can never matter:
// get_candidates only looks at segments whose index_score (own + left neighbour's seed count) reaches 2 * min_kmer_match
// (pw_impl.cpp:309) and, from those, at most ceil((L + 12) / 2000) segments to either side (:405-438).  With h(e) = bucket
// hits whose segment id is e modulo 2^15 (an upper bound of the seed count of every segment hashing to e), slot e is HOT
// when h(e) > 0 and h(e-1) + h(e) or h(e) + h(e+1) reaches the gate; a hit is kept when its slot lies within `sweep_reach`
// slots of a hot one.  Dropped hits touch no state that is ever read, so the result is unchanged: the filter only errs
// towards keeping (collisions inflate h and spread relevance).  One walk over the buckets fills the byte counters in LDS;
// hot slots, the relevance bitmap and the exact number of kept hits (sum of h over relevant slots: the strand's room in
// the key arrays) come from passes over the 32 K-entry table.  A counter that would wrap (>= 256 hits in one slot: repeats)
// turns the filter off for the strand.
__global__ __launch_bounds__(SEED_BLOCK) void seed_filter(const mhip_offset_t* __restrict__ roffs, ReadSel sel, int ib,
                                                          const uint16_t* __restrict__ slots, SeedArrays A, int gate, int enable) {
    static_assert(ZV == 2000 && FLT_M == (1 << 15), "idx_slots (index.hip) computes (position / 2000) mod 2^15");
    __shared__ uint32_t cnt[FLT_M / 4];          // 32 KB
    __shared__ uint32_t rel[REL_WORDS];          // 4 KB
    __shared__ uint32_t wtot[SEED_WAVES];
    __shared__ uint32_t s_wrap;
    const int s = blockIdx.x;
    const int rid = sel_rid(sel, ib + (s >> 1));
    const int L = roffs[rid].size;
    const int K = kmers_of(L);
    const uint32_t kb = A.km_base[s];
    const uint32_t Hall = A.strand_hits_all[s];
    if (A.fused[s]) {                 // done by seed_strand: nothing for the kernels of this path
        if (threadIdx.x == 0) { A.strand_hits[s] = 0; A.filtered[s] = 0; }
        return;
    }
    bool filtered = enable && Hall > 0;
    uint32_t kept = Hall;
    if (filtered) {
        for (int i = threadIdx.x; i < FLT_M / 4; i += SEED_BLOCK) cnt[i] = 0;
        for (int i = threadIdx.x; i < REL_WORDS; i += SEED_BLOCK) rel[i] = 0;
        if (threadIdx.x == 0) s_wrap = 0;
        __syncthreads();
        auto nop = [](int, int) {};
        for_each_hit16(A, slots, kb, K, nop, [&](int, int, uint32_t, uint32_t e, bool valid) {      // e = the hit's table slot
            if (valid) {
                const uint32_t sh = (e & 3u) * 8u;
                const uint32_t old = atomicAdd(&cnt[e >> 2], 1u << sh);
                if (((old >> sh) & 255u) == 255u) s_wrap = 1;
            }
        }, nop);
        __syncthreads();
        if (s_wrap) filtered = false;
    }
    if (filtered) {
        const uint8_t* cb = (const uint8_t*)cnt;
        const uint32_t reach = (uint32_t)min(sweep_reach(L), FLT_M / 2 - 1);
        for (int i = 0; i < FLT_M / SEED_BLOCK; ++i) {
            const uint32_t e = (uint32_t)i * SEED_BLOCK + threadIdx.x;
            const int c = cb[e];
            if (c > 0 && (c + (int)cb[(e + 1) & (FLT_M - 1)] >= gate || c + (int)cb[(e - 1) & (FLT_M - 1)] >= gate)) {
                uint32_t lo = (e - reach) & (FLT_M - 1), left = 2 * reach + 1;      // bits lo .. lo + left - 1, circular
                while (left > 0) {
                    const uint32_t b = lo & 31u, take = min(32u - b, left);
                    const uint32_t m = (take == 32u ? 0xFFFFFFFFu : ((1u << take) - 1u)) << b;
                    atomicOr(&rel[lo >> 5], m);
                    lo = (lo + take) & (FLT_M - 1);
                    left -= take;
                }
            }
        }
        __syncthreads();
        uint32_t mine = 0;
        for (int i = 0; i < FLT_M / SEED_BLOCK; ++i) {
            const uint32_t e = (uint32_t)i * SEED_BLOCK + threadIdx.x;
            if (rel_test(rel, e)) mine += cb[e];
        }
        uint32_t tot;
        (void)block_excl_scan(mine, wtot, &tot);
        kept = tot;
        for (int i = threadIdx.x; i < REL_WORDS; i += SEED_BLOCK) A.rel_bits[(size_t)s * REL_WORDS + i] = rel[i];
    }
    if (threadIdx.x == 0) { A.strand_hits[s] = kept; A.filtered[s] = filtered ? 1 : 0; }
}

#ifdef WF_PROF
// development build (make wfprof): s_memrealtime ticks per section of seed_filter_wide [0..7] and seed_emit [8..15], summed over strands
__device__ unsigned long long g_wfprof[16];
#define WF_MARK(i) do { __syncthreads(); if (threadIdx.x == 0) { const unsigned long long t_ = wall_clock64(); atomicAdd(&g_wfprof[i], t_ - t_prev); t_prev = t_; } } while (0)
#define WF_T0 unsigned long long t_prev = wall_clock64(); (void)t_prev
#else
#define WF_MARK(i) do { } while (0)
#define WF_T0
#endif
// ------------------------------------------------------------------------------------------------ relevance filter, low gates
// Nanopore mode gates at index_score >= 4 (min_kmer_match 2), and a 2.14 Gbase volume puts ~64 k bucket hits of a strand on ~1.07 M
// segments: folded onto seed_filter's 2^15 slots that is two hits per slot, every second slot pair passes a gate of 4, and the reach
// of the sweeps (+- 11 segments for a 20 kb read) makes everything relevant — which is why that filter is only used from a gate of 6
// up, and why nanopore strands used to sort and build all of their hits in HBM (0.66 of the 0.73 s of a config-5 grid cell).
// Same construction with 2^18 slots (a quarter hit per slot: 0.2 % of the slot pairs pass by chance) and 4-bit counters in the LDS of
// a whole CU; the relevance bitmap has one bit per 8 slots, so it is the 4 KB per strand seed_emit already reads.  A slot of a true
// overlap collects 20-30 hits, so a 4-bit counter wraps there: the add that wraps it (its return value says so, and which neighbours
// the carry ran into) marks the slot relevant on the spot and counts the wrap.  Counters next to a wrapped one are too high by the
// carry: the bitmap only grows, and the number of kept hits becomes an upper bound (sum over the relevant slots + 16 per wrap) — the
// room of the strand in the key arrays; seed_emit writes the exact number when it has placed the keys.
#ifndef WF_LPB
// the walk of seed_filter_wide: lanes per bucket, pieces loaded ahead, buckets per group and stage, stages in flight (see FS_LPB1)
#define WF_LPB 8
#define WF_NP 4
#define WF_Q 2
#define WF_D 2
#endif
#define WF_BITS 18
#define WF_M (1 << WF_BITS)
#define WF_CELL 3                    // log2 slots per relevance bit
static_assert((WF_M >> WF_CELL) == FLT_M, "the bitmap is REL_WORDS words");
__global__ __launch_bounds__(FS_THREADS) void seed_filter_wide(const mhip_offset_t* __restrict__ roffs, ReadSel sel, int ib,
                                                               const int32_t* __restrict__ offsets, SeedArrays A, int gate, int same_volume,
                                                               unsigned long long* __restrict__ counters) {
    __shared__ uint32_t cnt[WF_M / 8];           // 128 KB: eight 4-bit counters per word
    __shared__ uint32_t rel[REL_WORDS];
    __shared__ uint32_t hotb[3][REL_WORDS];      // cells with a hot slot; of those, the ones whose reach needs one more cell on the left / right
    __shared__ uint32_t wtot[FS_WAVES];
    __shared__ uint32_t s_wraps, s_self;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int rid = sel_rid(sel, ib + (s >> 1));
    const int L = roffs[rid].size;
    const int K = kmers_of(L);
    const uint32_t kb = A.km_base[s];
    const uint32_t Hall = A.strand_hits_all[s];
    if (A.fused[s] || Hall == 0) {
        if (tid == 0) { A.strand_hits[s] = 0; A.filtered[s] = 0; }
        return;
    }
    WF_T0;
    for (int i = tid; i < WF_M / 8; i += FS_THREADS) cnt[i] = 0;
    rel[tid] = 0;                                 // REL_WORDS == FS_THREADS
    static_assert(REL_WORDS == FS_THREADS, "one bitmap word per thread");
    if (tid == 0) { s_wraps = 0; s_self = 0; }
    __syncthreads();
    WF_MARK(0);
    const uint32_t reach = (uint32_t)min(sweep_reach(L), WF_M / 2 - 1);
    auto mark = [&](int lo, int hi) {            // slots lo .. hi (unwrapped, hi - lo < WF_M) -> their bitmap bits
        uint32_t cell = (uint32_t)(lo >> WF_CELL) & (FLT_M - 1), left = min((uint32_t)((hi >> WF_CELL) - (lo >> WF_CELL) + 1), (uint32_t)FLT_M);
        while (left > 0) {
            const uint32_t b = cell & 31u, take = min(32u - b, left);
            const uint32_t m = (take == 32u ? 0xFFFFFFFFu : ((1u << take) - 1u)) << b;
            atomicOr(&rel[cell >> 5], m);
            cell = (cell + take) & (FLT_M - 1);
            left -= take;
        }
    };
    // The forward strand of a read against the volume it comes from hits its own copy with every k-mer (200 hits per segment: every
    // counter there would wrap).  Those hits are known without counting them: position = the read's offset + 10 km.  They are
    // counted apart, and the read's own segments are relevant whatever the counters say.
    const bool own = same_volume && !(s & 1);
    const uint32_t own_off = (uint32_t)roffs[rid].offset;
    fs_walk<WF_LPB, WF_NP, WF_Q, WF_D, false>(tid, A.km_bstart + kb, A.km_cnt + kb, offsets, K, [&](int km, uint32_t pos) {
#if defined(WF_KNOCK) && WF_KNOCK == 1
        if (pos == 0xfffffff1u) atomicAdd(&s_self, 1u);      // timing experiment: the gather alone (results are wrong)
        return;
#elif defined(WF_KNOCK) && WF_KNOCK == 2
        { const uint32_t e_ = (pos / (uint32_t)ZV) & (WF_M - 1); atomicAdd(&cnt[e_ >> 3], 1u << ((e_ & 7u) * 4u)); return; }      // no return value, no wrap test
#endif
        if (own && pos == own_off + (uint32_t)km * BC) { atomicAdd(&s_self, 1u); return; }
        const uint32_t e = (pos / (uint32_t)ZV) & (WF_M - 1);
        const uint32_t old = atomicAdd(&cnt[e >> 3], 1u << ((e & 7u) * 4u));
        // the counters this add wrapped: slot e if it stood at 15, and the neighbours at 15 the carry went on through
        for (uint32_t n = e & 7u; n < 8u && ((old >> (4u * n)) & 15u) == 15u; ++n) {
            const int w = (int)((e & ~7u) + n);
            mark(w - (int)reach, w + (int)reach);
            atomicAdd(&s_wraps, 1u);
        }
    });
    __syncthreads();
    WF_MARK(1);
    // hot slots -> relevance bitmap (one bit per cell of 8 slots = one counter word)
    if (own && tid == 0) mark((int)(own_off / (uint32_t)ZV) - (int)reach, (int)((own_off + (uint32_t)L) / (uint32_t)ZV) + (int)reach);
    {
        // Eight counters at a time: the even and the odd nibbles of a word as the bytes of two registers, the four sums inside the pairs
        // (n0+n1 ..) and the four across them (n1+n2 .., n7 + the next word's n0) as byte adds, "sum >= gate" as the carry into bit 7 of
        // every byte (sums are at most 30).  A slot is hot when it is occupied and one of its two pairs reaches the gate.  All hot slots
        // of a word lie in one bitmap cell c, and with reach = 8 a + b their reaches cover the cells c - a .. c + a, one more on the left
        // when the lowest hot slot of the word is below b, one more on the right when the highest is at 8 - b or above: three cell
        // bitmaps (hot, needs-left, needs-right), written as wave ballots (lanes = consecutive words: a thread that walks 32 consecutive
        // words of its own puts all 64 lanes of every read on one LDS bank), and one dilation pass, thread t = bitmap word t.
        // (Slot by slot, a branch per nibble and an atomicOr loop per hot slot: 22 of the kernel's 56 us per strand; this: 4.)
        const uint32_t kb7 = (uint32_t)(128 - min(gate, 31)) * 0x01010101u;
        const int ra = (int)(reach >> 3), rb = (int)(reach & 7u);
        const bool by_bitmaps = ra <= 16;            // (longer reaches — reads beyond 250 kb — mark hot word by hot word)
#pragma unroll 4
        for (int j = 0; j < 32; ++j) {
            const uint32_t wi = (uint32_t)(j * FS_THREADS + tid);
            // (all three reads unconditionally: no branch in front of the arithmetic, the reads of the unrolled steps overlap)
            const uint32_t w = cnt[wi], wprev = cnt[(wi - 1u) & (WF_M / 8 - 1)], wnext = cnt[(wi + 1u) & (WF_M / 8 - 1)];
            const uint32_t E = w & 0x0F0F0F0Fu, O = (w >> 4) & 0x0F0F0F0Fu;
            // bit 7 of every byte: the pair's sum reaches the gate / the counter is not zero
            const uint32_t H1 = E + O + kb7;                                                              // pairs (0,1) (2,3) (4,5) (6,7)
            const uint32_t H2 = O + __builtin_amdgcn_alignbit(wnext & 15u, E, 8) + kb7;                   // pairs (1,2) (3,4) (5,6) (7,next)
            const uint32_t hp = ((wprev >> 28) + (w & 15u)) >= (uint32_t)gate ? 0x80u : 0u;              // pair (previous word's 7, 0)
            const uint32_t hotE = (E + 0x7F7F7F7Fu) & (H1 | (H2 << 8) | hp) & 0x80808080u;
            const uint32_t hotO = (O + 0x7F7F7F7Fu) & (H1 | H2) & 0x80808080u;
            const uint32_t m = (hotE >> 7) | (hotO >> 6);          // bit 8 i + j <-> nibble 2 i + j
            const unsigned long long bh = __ballot(m != 0);
            if (by_bitmaps) {
                unsigned long long bl = 0, br = 0;
                if (bh) {               // (a wave with a hot word: one step in ten)
                    const int l = __builtin_ctz(m | 0x80000000u), h = 31 - __builtin_clz(m | 1u);
                    const int lo = ((l >> 3) << 1) | (l & 1), hi = ((h >> 3) << 1) | (h & 1);
                    bl = __ballot(m != 0 && lo < rb); br = __ballot(m != 0 && hi + rb >= 8);
                }
                if ((tid & 63) == 0) {
                    const uint32_t bw = wi >> 5;          // the wave's 64 words = two bitmap words
                    hotb[0][bw] = (uint32_t)bh; hotb[0][bw + 1] = (uint32_t)(bh >> 32);
                    hotb[1][bw] = (uint32_t)bl; hotb[1][bw + 1] = (uint32_t)(bl >> 32);
                    hotb[2][bw] = (uint32_t)br; hotb[2][bw + 1] = (uint32_t)(br >> 32);
                }
            } else if (m) {
                const int l = __builtin_ctz(m), h = 31 - __builtin_clz(m);
                const int e0 = (int)wi * 8;
                mark(e0 + (((l >> 3) << 1) | (l & 1)) - (int)reach, e0 + (((h >> 3) << 1) | (h & 1)) + (int)reach);
            }
        }
        if (by_bitmaps) {
            __syncthreads();
            // word t of bitmap B moved d cells up (d < 0: down), circular
            auto moved = [&](const uint32_t* B, int d) -> uint32_t {
                if (d >= 0) {
                    const int q = d >> 5, r = d & 31;
                    const uint32_t x = B[(tid - q) & (REL_WORDS - 1)];
                    return r ? (x << r) | (B[(tid - q - 1) & (REL_WORDS - 1)] >> (32 - r)) : x;
                }
                const int q = (-d) >> 5, r = (-d) & 31;
                const uint32_t x = B[(tid + q) & (REL_WORDS - 1)];
                return r ? (x >> r) | (B[(tid + q + 1) & (REL_WORDS - 1)] << (32 - r)) : x;
            };
            uint32_t acc = moved(hotb[2], ra + 1) | moved(hotb[1], -(ra + 1));
            for (int d = -ra; d <= ra; ++d) acc |= moved(hotb[0], d);
            if (acc) atomicOr(&rel[tid], acc);          // (the wraps of the walk and the read's own segments are in there already)
        }
    }
    __syncthreads();
    WF_MARK(2);
    // kept hits = hits of the slots whose bit is set
    uint32_t mine = 0;
    {
        const uint32_t r = rel[tid];
        for (uint32_t m = r; m; m &= m - 1u) {
            const uint32_t w = cnt[32 * tid + (uint32_t)__builtin_ctz(m)];
            // sum of the eight nibbles
            const uint32_t a = (w & 0x0F0F0F0Fu) + ((w >> 4) & 0x0F0F0F0Fu);
            mine += (a * 0x01010101u) >> 24;
        }
    }
    uint32_t kept;
    (void)fs_excl_scan(tid, mine, wtot, &kept);
    A.rel_bits[(size_t)s * REL_WORDS + tid] = rel[tid];
    if (tid == 0) {
        const uint32_t room = min(Hall, kept + s_self + 16u * s_wraps);
        A.strand_hits[s] = room;
        A.filtered[s] = 1;
        atomicAdd(&counters[12], (unsigned long long)room);      // debug slot 12: room asked for by this filter
    }
    WF_MARK(3);
}

// ------------------------------------------------------------------------------------------------ emit
// keys of the kept hits in (km, position) order = the order the reference visits them: key = seg:21 | km:16 | off:11.
// The strand's k-mers are taken 64 at a time (16 lanes per bucket, four buckets per group as in for_each_hit16): count the
// kept hits per bucket, scan the 64 counts, write.  The first 32 entries of a bucket stay in registers between the two
// steps; longer buckets are read again (from cache).
#ifndef EMIT_NP
#define EMIT_NP 4                     // 16-entry pieces of a bucket loaded together (the rest, if any, one by one)
#endif
__global__ __launch_bounds__(SEED_BLOCK) void seed_emit(const mhip_offset_t* __restrict__ roffs, ReadSel sel, int ib,
                                                        const int32_t* __restrict__ offsets, SeedArrays A) {
    __shared__ uint32_t rel[REL_WORDS];
    __shared__ uint32_t ccnt[64];
    __shared__ uint32_t coff[64];
    __shared__ uint32_t s_tot;
    const int s = blockIdx.x;
    const int rid = sel_rid(sel, ib + (s >> 1));
    const int L = roffs[rid].size;
    const int K = kmers_of(L);
    const uint32_t kb = A.km_base[s];
    if (A.strand_hits[s] == 0) return;
    WF_T0;
    uint64_t* __restrict__ out = A.keysA + A.hit_base[s];
    const bool flt = A.filtered[s] != 0;
    if (flt) {
        for (int i = threadIdx.x; i < REL_WORDS; i += SEED_BLOCK) rel[i] = A.rel_bits[(size_t)s * REL_WORDS + i];
    }
    __syncthreads();
    WF_MARK(8);
    const int g = threadIdx.x >> 4;
    const uint32_t sub = threadIdx.x & 15;
    const uint32_t below = (1u << sub) - 1u;
    uint32_t run = 0;
    // EMIT_NP pieces of 16 entries of every bucket are requested together, before any is used: a piece that is loaded when the one in
    // front of it has been consumed costs the group a memory latency of its own, and at nanopore volume sizes (32 entries per bucket on
    // average, many at the cap of 128) those serial loads — in a wave, whenever one of its four groups has a long bucket — were the
    // kernel's time.  The verdict of the count pass on each entry of those pieces stays in a register for the write pass.
    for (int c0 = 0; c0 < K; c0 += 64) {
        uint32_t bs[4], cn[4], pc[4][EMIT_NP];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int km = c0 + q * 16 + g;
            bs[q] = km < K ? A.km_bstart[kb + km] : 0u;
            cn[q] = km < K ? A.km_cnt[kb + km] : 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int p = 0; p < EMIT_NP; ++p) pc[q][p] = sub + 16u * p < cn[q] ? (uint32_t)offsets[bs[q] + 16 * p + sub] : 0u;
        // count
        uint32_t keep = 0;          // bit EMIT_NP q + p: this lane's entry of piece p of bucket q is kept
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t kept = 0;
#pragma unroll
            for (int p = 0; p < EMIT_NP; ++p)
                if (16u * p < cn[q]) {
                    const bool k1 = sub + 16u * p < cn[q] && (!flt || rel_test(rel, pc[q][p] / ZV, A.rel_mask, A.rel_shift));
                    kept += __popc(group_bits(__ballot(k1)));
                    keep |= k1 ? 1u << (EMIT_NP * q + p) : 0u;
                }
            for (uint32_t r0 = 16 * EMIT_NP; r0 < cn[q]; r0 += 16) {
                const uint32_t r = r0 + sub;
                const bool valid = r < cn[q];
                const uint32_t pos = valid ? (uint32_t)offsets[bs[q] + r] : 0u;
                kept += __popc(group_bits(__ballot(valid && (!flt || rel_test(rel, pos / ZV, A.rel_mask, A.rel_shift)))));
            }
            if (sub == 0) ccnt[q * 16 + g] = kept;
        }
        __syncthreads();
        WF_MARK(9);
        if (threadIdx.x < 64) {
            const uint32_t v = ccnt[threadIdx.x];
            uint32_t incl = v;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t nb = __shfl_up(incl, o);
                if ((int)threadIdx.x >= o) incl += nb;
            }
            coff[threadIdx.x] = incl - v;
            if (threadIdx.x == 63) s_tot = incl;
        }
        __syncthreads();
        WF_MARK(10);
        // write
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int km = c0 + q * 16 + g;
            uint32_t at = run + coff[q * 16 + g];
            auto put = [&](uint32_t pos, bool k1) {
                const uint32_t seg = pos / ZV, so = pos - seg * ZV;
                const uint32_t bits = group_bits(__ballot(k1));
                if (k1) out[at + __popc(bits & below)] = ((uint64_t)seg << KEY_SEG_SHIFT) | ((uint64_t)km << KEY_OFF_BITS) | so;
                at += __popc(bits);
            };
#pragma unroll
            for (int p = 0; p < EMIT_NP; ++p)
                if (16u * p < cn[q]) put(pc[q][p], (keep >> (EMIT_NP * q + p)) & 1u);
            for (uint32_t r0 = 16 * EMIT_NP; r0 < cn[q]; r0 += 16) {
                const uint32_t r = r0 + sub;
                const bool valid = r < cn[q];
                const uint32_t pos = valid ? (uint32_t)offsets[bs[q] + r] : 0u;
                put(pos, valid && (!flt || rel_test(rel, pos / ZV, A.rel_mask, A.rel_shift)));
            }
        }
        WF_MARK(11);
        run += s_tot;
    }
    // the number of keys written: exact, where seed_filter_wide's strand_hits was the room it asked for (an upper bound)
    if (threadIdx.x == 0) A.strand_hits[s] = run;
}

// ------------------------------------------------------------------------------------------------ sort (one LSD pass)
// digit = (key >> shift) & (2^bits - 1), bits <= SORT_MAXBITS (two passes cover the 20-21 segment bits of a volume).  Wave w
// of the block owns the w-th quarter of the strand's keys.
#define SORT_MAXBITS 11
#define SORT_BINS (1 << SORT_MAXBITS)
__global__ __launch_bounds__(SEED_BLOCK) void seed_sort_pass(SeedArrays A, int from_b, int shift, int bits) {
    __shared__ uint32_t hist[SEED_WAVES][SORT_BINS];      // 32 KB
    __shared__ uint32_t wtot[SEED_WAVES];
    const int s = blockIdx.x;
    const uint32_t H = A.strand_hits[s];
    if (H == 0) return;
    const uint64_t hb = A.hit_base[s];
    const uint64_t* __restrict__ src = (from_b ? A.keysB : A.keysA) + hb;
    uint64_t* __restrict__ dst = (from_b ? A.keysA : A.keysB) + hb;
    const int w = threadIdx.x >> 6, lane = lane_id();
    const uint32_t mask = (1u << bits) - 1u;
    const uint32_t chunk = (((H + SEED_WAVES - 1) / SEED_WAVES) + 63u) & ~63u;
    const uint32_t lo = min(H, w * chunk), hi = min(H, lo + chunk);
    const uint32_t nbins = 1u << bits;
    for (uint32_t i = threadIdx.x; i < nbins; i += SEED_BLOCK)
#pragma unroll
        for (int q = 0; q < SEED_WAVES; ++q) hist[q][i] = 0;
    __syncthreads();
    for (uint32_t i = lo + lane; i < hi; i += 64) atomicAdd(&hist[w][(uint32_t)(src[i] >> shift) & mask], 1u);
    __syncthreads();
    {
        // bases in (bin major, wave minor) order, SEED_BLOCK bins per round
        uint32_t carry = 0;
        for (uint32_t b0 = 0; b0 < nbins; b0 += SEED_BLOCK) {
            const uint32_t bin = b0 + threadIdx.x;
            const bool in = bin < nbins;
            uint32_t c[SEED_WAVES], tot = 0;
#pragma unroll
            for (int q = 0; q < SEED_WAVES; ++q) { c[q] = in ? hist[q][bin] : 0u; tot += c[q]; }
            uint32_t all;
            uint32_t ex = carry + block_excl_scan(tot, wtot, &all);
            if (in) {
#pragma unroll
                for (int q = 0; q < SEED_WAVES; ++q) { hist[q][bin] = ex; ex += c[q]; }
            }
            carry += all;
        }
    }
    __syncthreads();
    volatile uint32_t* cur = hist[w];
    const uint64_t lt = (1ull << lane) - 1ull;
    for (uint32_t i0 = lo; i0 < hi; i0 += 64) {
        uint32_t i = i0 + lane;
        bool valid = i < hi;
        uint64_t key = valid ? src[i] : 0;
        uint32_t d = (uint32_t)(key >> shift) & mask;
        uint64_t peers = __ballot(valid);
        for (int b = 0; b < bits; ++b) {
            uint64_t m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        uint32_t rank = __popcll(peers & lt);
        uint32_t base = valid ? cur[d] : 0;
        if (valid) dst[base + rank] = key;
        if (valid && rank == 0) cur[d] = base + (uint32_t)__popcll(peers);
    }
}

// ------------------------------------------------------------------------------------------------ build
__global__ __launch_bounds__(SEED_BLOCK) void seed_build(SeedArrays A, int sorted_in_b, int min_kmer_match, double cutoff, ReadSel sel, int ib,
                                                         RefReads R) {
    __shared__ uint32_t wtot[SEED_WAVES];
    __shared__ uint32_t s_cnt[4];          // 0: overflow count, 1: gated count
    __shared__ uint64_t s_tf[GATE_LDS];    // first-touch times of the gated segments (phase E)
    const int s = blockIdx.x;
    const uint32_t H = A.strand_hits[s];
    const int own_rid = sel_rid(sel, ib + (s >> 1));
    const int own_end = R.same_volume ? R.offs[own_rid].offset + R.offs[own_rid].size + 1 : 0;
    const uint64_t hb = A.hit_base[s];
    if (H == 0) {
        if (threadIdx.x == 0) { A.nseg[s] = 0; A.nrec[s] = 0; A.ngated[s] = 0; }
        return;
    }
    const uint64_t* __restrict__ S = (sorted_in_b ? A.keysB : A.keysA) + hb;
    uint32_t* ovf_list = (uint32_t*)((sorted_in_b ? A.keysA : A.keysB) + hb);   // free sort buffer: overflow work list
    uint64_t* gate_tmp = (sorted_in_b ? A.keysA : A.keysB) + hb;                // later: unsorted gated keys
    uint32_t* ent = A.ent + hb;
    uint32_t* fin = A.ent_fin + hb;
    uint16_t* esc = A.escore + hb;
    uint32_t* seg_id = A.seg_id + hb;
    uint32_t* seg_start = A.seg_start + hb;
    int32_t* seg_score = A.seg_score + hb;
    uint32_t* seg_kmlast = A.seg_kmlast + hb;
    uint64_t* seg_tfirst = A.seg_tfirst + hb;
    uint32_t* gated = A.gated + hb;

    // ---- phase A: recorded events and segment heads
    uint32_t rec_run = 0, seg_run = 0;
    for (uint32_t t0 = 0; t0 < H; t0 += SEED_BLOCK) {
        uint32_t i = t0 + threadIdx.x;
        bool in = i < H;
        uint64_t key = in ? S[i] : 0, prev = (in && i > 0) ? S[i - 1] : 0;
        bool head = in && (i == 0 || key_seg(key) != key_seg(prev));
        // a hit is recorded when the segment is new or its last seed number is below this k-mer's (pw_impl.cpp:265): the first hit of each
        // (segment, km) — until the reference's `short seednum` wraps: from seed number 32 768 on (reads beyond 327 670 bases) it is
        // negative, below every k-mer number, and every further hit of the segment is recorded
        bool rec = in && (head || key_km(key) != key_km(prev) || key_km(prev) >= 32767u);
        // one scan for both counts: recorded events in the low half, segment heads in the high half (<= 256 each per round)
        uint32_t both;
        const uint32_t ex = block_excl_scan((rec ? 1u : 0u) | (head ? 0x10000u : 0u), wtot, &both);
        const uint32_t rtot = both & 0xFFFFu, stot = both >> 16;
        uint32_t rpos = rec_run + (ex & 0xFFFFu);
        uint32_t spos = seg_run + (ex >> 16);
        if (rec) ent[rpos] = (key_off(key) << 16) | ((key_km(key) + 1u) & 0xFFFFu);
        if (head) {
            seg_id[spos] = key_seg(key);
            seg_start[spos] = rpos;
            seg_tfirst[spos] = ((uint64_t)key_km(key) << 32) | (uint64_t)(key_seg(key) * (uint32_t)ZV + key_off(key));
            if (spos > 0) seg_kmlast[spos - 1] = key_km(prev);
        }
        rec_run += rtot;
        seg_run += stot;
    }
    const uint32_t nrec = rec_run, nseg = seg_run;
    if (threadIdx.x == 0) {
        seg_kmlast[nseg - 1] = key_km(S[H - 1]);
        A.nseg[s] = nseg;
        A.nrec[s] = nrec;
        s_cnt[0] = 0;
        s_cnt[1] = 0;
    }
    __syncthreads();

    // ---- phase B: scores; collect overflowed segments
    for (uint32_t g = threadIdx.x; g < nseg; g += SEED_BLOCK) {
        uint32_t st = seg_start[g], en = (g + 1 < nseg) ? seg_start[g + 1] : nrec;
        uint32_t c = en - st;
        if (c > SM) { uint32_t k = atomicAdd(&s_cnt[0], 1u); ovf_list[k] = g; seg_score[g] = OVF_FLAG; }
        else seg_score[g] = (int32_t)c;
    }
    __syncthreads();

    // ---- phase C: replay insert_loc, one wave per overflowed segment
    {
        const uint32_t novf = s_cnt[0];
        for (uint32_t k = threadIdx.x >> 6; k < novf; k += SEED_WAVES) {
            uint32_t g = ovf_list[k];
            uint32_t st = seg_start[g], en = (g + 1 < nseg) ? seg_start[g + 1] : nrec;
            int sc;
            replay_overflow(ent + st, (int)(en - st), fin + st, esc + st, cutoff, &sc);
            if (lane_id() == 0) seg_score[g] = sc | OVF_FLAG;
        }
    }
    __syncthreads();

    // ---- phase D: index_score = own score + left neighbour's score at the time of the last event (pw_impl.cpp:270-280)
    for (uint32_t g = threadIdx.x; g < nseg; g += SEED_BLOCK) {
        int own = seg_score[g] & ~OVF_FLAG;
        int s_k = own;
        uint32_t sid = seg_id[g];
        if (g > 0 && sid > 0 && seg_id[g - 1] == sid - 1) {
            // events of the left neighbour with km <= km_last happened before this segment's last event
            uint32_t st = seg_start[g - 1], en = seg_start[g];
            uint32_t t = seg_kmlast[g] + 1u;     // compare on km + 1 as stored
            uint32_t lo = st, hi = en;           // first event with (km + 1) > t
            while (lo < hi) {
                uint32_t mid = (lo + hi) >> 1;
                if ((ent[mid] & 0xFFFFu) <= t) lo = mid + 1; else hi = mid;
            }
            int left = 0;
            if (lo > st) left = (seg_score[g - 1] & OVF_FLAG) ? (int)esc[lo - 1] : (int)(lo - st);
            s_k += left;
        }
        if ((int)(int16_t)s_k >= 2 * min_kmer_match && !(R.enable && subjects_all_higher(R, sid, own_rid, own_end))) {
            uint32_t k = atomicAdd(&s_cnt[1], 1u);
            gate_tmp[k] = (uint64_t)g;   // index only; ordered below by seg_tfirst
        }
    }
    __syncthreads();

    // ---- phase E: order gated segments by first-touch time (rank sort; first-touch times are unique)
    {
        const uint32_t ng = s_cnt[1];
        if (ng <= GATE_LDS) {       // the usual case (~250 gated segments): times staged in LDS, ranks from broadcast reads
            for (uint32_t a = threadIdx.x; a < ng; a += SEED_BLOCK) s_tf[a] = seg_tfirst[(uint32_t)gate_tmp[a]];
            __syncthreads();
            for (uint32_t a = threadIdx.x; a < ng; a += SEED_BLOCK) {
                const uint64_t ta = s_tf[a];
                uint32_t rank = 0;
                for (uint32_t b = 0; b < ng; ++b) rank += s_tf[b] < ta ? 1u : 0u;
                gated[rank] = (uint32_t)gate_tmp[a];
            }
        } else {
            for (uint32_t a = threadIdx.x; a < ng; a += SEED_BLOCK) {
                uint32_t ga = (uint32_t)gate_tmp[a];
                uint64_t ta = seg_tfirst[ga];
                uint32_t rank = 0;
                for (uint32_t b = 0; b < ng; ++b) rank += seg_tfirst[(uint32_t)gate_tmp[b]] < ta ? 1u : 0u;
                gated[rank] = ga;
            }
        }
        if (threadIdx.x == 0) A.ngated[s] = ng;
    }
}

// ------------------------------------------------------------------------------------------------ launchers
// The bucket headers of every query k-mer (km_bstart, km_cnt: 8 bytes per lookup), for the whole batch.  tally = 0: seed_strand has
// counted these lookups already and only the km_* arrays are wanted.
int seed_run_probe(SeedBatch& b, int tally) {
    mhip_ctx* c = b.c;
    if (c->scratch("sd_kmbstart", sizeof(uint32_t) * (size_t)(b.sumK + 1), (void**)&b.A.km_bstart)) return -1;
    if (c->scratch("sd_kmcnt", sizeof(uint32_t) * (size_t)(b.sumK + 1), (void**)&b.A.km_cnt)) return -1;
    LAUNCH(c, "seed_probe", seed_probe, b.ns, SEED_BLOCK, 0, (const uint32_t*)b.reads->d_pac, (const mhip_offset_t*)b.reads->d_offs, b.sel, b.ib,
           (const uint32_t*)b.idx->d_starts, b.A, (unsigned long long*)c->d_counters, b.recs, b.cut_step, tally);
    return 0;
}

// kept hits per strand: the filter of the batch's gate (with the low gates of nanopore mode seed_filter_wide)
static int chain_filter(SeedBatch& b) {
    mhip_ctx* c = b.c;
    SeedArrays& B = b.B;
    const int ns = b.ns;
    if (seed_strand_tables(c, "sd_", ns, &B)) return -1;
    if (c->scratch("sd_filtered", sizeof(int32_t) * (size_t)ns, (void**)&B.filtered)) return -1;
    if (c->scratch("sd_relbits", sizeof(uint32_t) * (size_t)ns * REL_WORDS, (void**)&B.rel_bits)) return -1;
    if (b.knobs.wide_filter) {           // low gates (nanopore mode): 2^18 slots, one workgroup per strand and CU
        B.rel_mask = WF_M - 1;
        B.rel_shift = WF_CELL;
        LAUNCH(c, "seed_filter_wide", seed_filter_wide, ns, FS_THREADS, 0, (const mhip_offset_t*)b.reads->d_offs, b.sel, b.ib,
               (const int32_t*)b.idx->d_offsets, B, b.gate, b.ref == b.reads ? 1 : 0, (unsigned long long*)c->d_counters);
    } else {
        B.rel_mask = FLT_M - 1;
        B.rel_shift = 0;
        LAUNCH(c, "seed_filter", seed_filter, ns, SEED_BLOCK, 0, (const mhip_offset_t*)b.reads->d_offs, b.sel, b.ib,
               (const uint16_t*)b.idx->d_slots, B, b.gate, b.knobs.filter ? 1 : 0);
    }
    return 0;
}

// region of every strand in the per-hit tables; the host waits for their size (the second of a batch's two waits)
static int chain_room(SeedBatch& b, uint64_t* Htot) {
    mhip_ctx* c = b.c;
    SeedArrays& B = b.B;
    LAUNCH(c, "seed_scan", seed_scan, 1, 1024, 0, (const uint32_t*)B.strand_hits, b.ns, B.hit_base);
    HIPCHK(hipMemcpyAsync(Htot, B.hit_base + b.ns, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t Hc = (size_t)*Htot + 64;
    if (c->scratch("sd_keysA", sizeof(uint64_t) * Hc, (void**)&B.keysA)) return -1;
    if (c->scratch("sd_keysB", sizeof(uint64_t) * Hc, (void**)&B.keysB)) return -1;
    if (seed_hit_tables(c, "sd_", Hc, &B)) return -1;
    if (c->scratch("sd_segkmlast", sizeof(uint32_t) * Hc, (void**)&B.seg_kmlast)) return -1;
    if (c->scratch("sd_segtfirst", sizeof(uint64_t) * Hc, (void**)&B.seg_tfirst)) return -1;
    return 0;
}

#ifdef WF_PROF
static int wf_prof_print(mhip_ctx* c, int ns) {
    unsigned long long h[16], z[16] = {0};
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_wfprof), sizeof(h)));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_wfprof), z, sizeof(z)));
    const char* nm[16] = {"wf zero", "wf walk", "wf hot", "wf kept+out", 0, 0, 0, 0, "emit bitmap", "emit load+count", "emit scan", "emit write"};
    for (int i = 0; i < 16; ++i) if (nm[i]) fprintf(stderr, "[wf prof] %-16s %8.1f us per strand (%d strands)\n", nm[i], (double)h[i] / 100.0 / ns, ns);
    return 0;
}
#endif

// keys of the kept hits, sorted by segment: -> 1 when the sorted keys are in keysB
static int chain_emit_sort(SeedBatch& b, int* in_b) {
    mhip_ctx* c = b.c;
    LAUNCH(c, "seed_emit", seed_emit, b.ns, SEED_BLOCK, 0, (const mhip_offset_t*)b.reads->d_offs, b.sel, b.ib, (const int32_t*)b.idx->d_offsets, b.B);
#ifdef WF_PROF
    if (wf_prof_print(c, b.ns)) return -1;
#endif
    const int npass = (b.nbits + SORT_MAXBITS - 1) / SORT_MAXBITS;
    const int per = (b.nbits + npass - 1) / npass;
    int done = 0;
    for (int p = 0; p < npass; ++p) {
        int bits = std::min(per, b.nbits - done);
        LAUNCH(c, "seed_sort_pass", seed_sort_pass, b.ns, SEED_BLOCK, 0, b.B, *in_b, KEY_SEG_SHIFT + done, bits);
        done += bits;
        *in_b ^= 1;
    }
    return 0;
}

// the kernel chain for the strands seed_strand did not build (A.fused[s] == 0); needs the km_* arrays of seed_run_probe in B
int seed_run_chain(SeedBatch& b) {
    uint64_t Htot = 0;
    int in_b = 0;
    if (chain_filter(b)) return -1;
    if (chain_room(b, &Htot)) return -1;
    if (Htot > 0 && chain_emit_sort(b, &in_b)) return -1;
    LAUNCH(b.c, "seed_build", seed_build, b.ns, SEED_BLOCK, 0, b.B, in_b, (int)b.P->min_kmer_match, b.P->ddfs_cutoff, b.sel, b.ib, b.RR);
    return 0;
}
