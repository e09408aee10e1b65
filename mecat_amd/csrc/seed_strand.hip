// seed_strand.hip — the strand-resident pipeline of the seeding stage and its launcher (seed.hip describes the stage and which strand
// takes this pipeline)
#include <stdlib.h>

#include <algorithm>

#include "seed_defs.h"
#include "seed_replay.h"
#include "seed_walk.h"

// ------------------------------------------------------------------------------------------------ the strand-resident pipeline
// seed_strand = seed_filter + seed_emit + seed_sort_pass x 2 + seed_build of one strand inside one workgroup, for the strands whose
// kept hits fit the LDS of a CU (all of them at BASELINE config 2: ~4 k kept hits of ~39 k bucket hits per strand, ~2.7 k
// segments).  The kept hits never travel through HBM: what leaves the workgroup is what seed_cand reads (recorded events, the
// segment table in ascending segment order, the gated segments in first-touch order).  Everything else falls back to the
// kernels above, strand by strand (A.fused[s] == 0): nanopore mode (no relevance filter), strands with more than FS_CAP kept
// hits or FS_SEGCAP segments, repeats that pile > FS_BIGN hits into one table slot, and strands that find the shared output
// arrays full.
//
//   walk 1  (slots[])    16-bit hit counters per hashed segment id ("table slot", 2^15 of them), LDS atomics, no return value
//   relevance            as seed_filter; then occ = relevant & non-empty slots, compact index ci(slot) = word prefix + popcount,
//                        region start of every occupied slot = prefix sum of its counter
//   walk 2  (offsets[])  every kept hit takes the next place of its slot's region (LDS atomic): payload = seg_hi:6 | km:15 |
//                        off:11, slot kept beside it.  Regions come out in slot order; inside a region the order is whatever
//                        the atomics made it
//   region sort          ascending payload inside each region = (segment, km, position) order, the order the reference visits
//                        the hits of a segment in (keys are unique).  Regions are tiny (a hit or two) except where a read
//                        meets itself (~200 hits per segment): every element of a short region counts the smaller ones (all reads,
//                        barrier, all writes); a wave sorts a long region in registers (bitonic network)
//   build                phases A-E of seed_build on the LDS arrays.  The elements stay in slot-major order; only the segment
//                        table is permuted to ascending segment id (stable split on the segment bits above the slot bits)
//
// Both walks are software pipelined: bucket headers two steps ahead, bucket data one step ahead of the hits being consumed.
// They are gathers of ~50 / ~90 byte runs (mecat_amd/tools/gather_peak.hip measures what the chip delivers on such runs: 35 G / s of
// <= 64 bytes, 26 G / s of 128 bytes), and they cost per bucket rather than per hit: see the FS_LPB / FS_NP table below.
#define FS_CAP 8192                  // kept hits
#define FS_SEGCAP 6144               // segments
#define FS_SMALLN 16                 // regions up to this length: every element ranks itself
#define FS_BIGN 512                  // longest region (8 elements per lane of a wave)
#define FS_BIGCAP 768                // regions longer than FS_SMALLN (FS_CAP / (FS_SMALLN + 1) at most: 630)
#define FS_GATECAP 1024              // gated segments
#define FS_OVF16 0x8000u
#ifndef FS_Q1
// walk 1 / walk 2: lanes per bucket, pieces of a bucket loaded ahead, buckets per group and stage, stages in flight.  Measured at
// config 2 (seed_strand per pass): 16 lanes x 3 pieces 46.1 ms, 8 x 4 43.4 ms, 8 x 3 45.0, 8 x 2 48.9, 4 x 8 50.4; three buckets per
// stage or three stages in flight 45.3 - 45.8: a walk costs per bucket (its loads are issued whatever the bucket holds), not per hit
#define FS_LPB1 8
#define FS_NP1 4
#define FS_Q1 2
#define FS_D1 2
#define FS_LPB2 8
#define FS_NP2 4
#define FS_Q2 2
#define FS_D2 2
#endif

struct FsLds {
    union {
        uint32_t cnt32[FLT_M / 2];                       // walk 1 .. relevance: 16-bit counters, two per word (64 KB)
        struct {
            uint32_t pay[FS_CAP];                        // walk 2 ..: payload, then (phase A, in place) recorded events
            uint16_t eslot[FS_CAP];
            uint16_t big[FS_BIGCAP];                     // long regions (compact slot index); later: overflowed segments
            uint32_t hist[FS_WAVES][64];                 // segment permutation: per-wave cursors
            uint64_t tf[FS_GATECAP];                     // first-touch times of the gated segments
        } e;
    } x;
    union {
        uint32_t cur32[FS_CAP / 2];                      // region cursors, 16 bit each (walk 2, region sort)
        uint16_t perm[FS_SEGCAP];                        // build: segment-order index -> slot-order index
    } y;
    uint32_t occ[REL_WORDS];
    uint32_t rel[REL_WORDS];
    uint16_t base_ci[REL_WORDS];
    uint32_t sq_id[FS_SEGCAP];                           // segment table in slot-major order q; until phase A: bucket start of every k-mer
    uint16_t sq_st[FS_SEGCAP + 2];                       // first recorded event of the segment; [nseg] = nrec
    uint16_t sq_score[FS_SEGCAP];                        // live score | FS_OVF16; until phase B: bucket size of every k-mer
    uint16_t gate[FS_GATECAP];
    uint32_t qpos[FS_WAVES][128];                        // walk 2: kept hits waiting for a full wave (position, km)
    uint16_t qkm[FS_WAVES][128];
    uint32_t wtot[FS_WAVES];
    unsigned long long red[FS_WAVES];                    // fs_block_sum2
    unsigned long long tally[3];                         // the workgroup's share of counters[0], [1], [15] (thread 0)
    uint32_t misc[12];                                   // 0 big count, 1 overflow count, 2 gated count, 3 fail flag, 4/5 carry, 6 hb lo, 7 hb hi,
                                                         // 8 / 9 strands taken from the cursor (not cleared between strands)
};
static_assert(sizeof(FsLds) <= 160 * 1024 - 512, "one workgroup per CU");

struct FusedCtl { unsigned long long alloc; unsigned int n_fallback; unsigned int next /* strand cursor */; unsigned long long prof[32]; };
#ifdef FS_PROF
#define FS_MARK(i) do { __syncthreads(); if (threadIdx.x == 0) { const unsigned long long t_ = wall_clock64(); atomicAdd(&ctl->prof[(i) + 16 * (s & 1)], t_ - t_prev); t_prev = t_; } } while (0)
#else
#define FS_MARK(i) do { } while (0)
#endif

// block-wide sums of two values per thread, FS_THREADS threads (a barrier inside: what was written to LDS before the call is visible after it)
__device__ __forceinline__ void fs_block_sum2(const int tid, uint32_t a, uint32_t b, unsigned long long* red /*[FS_WAVES]*/, uint32_t* sa, uint32_t* sb) {
    const int lane = tid & 63;
    for (int o = 32; o > 0; o >>= 1) {
        a += (uint32_t)__builtin_amdgcn_ds_bpermute((lane ^ o) << 2, (int)a);
        b += (uint32_t)__builtin_amdgcn_ds_bpermute((lane ^ o) << 2, (int)b);
    }
    const unsigned long long v = (unsigned long long)a | ((unsigned long long)b << 32);      // (each wave's sums are below 2^32)
    if (lane == 0) red[tid >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < FS_WAVES; ++w) t += red[w];
    *sa = (uint32_t)t;
    *sb = (uint32_t)(t >> 32);
}

// What seed_probe computes per query k-mer, in the two dependent steps seed_strand issues apart: the two packed words that hold the
// k-mer, then the bucket's record (the cut record of a diagonal cell, or starts[id] and starts[id + 1]), kept raw until it is needed.
struct FsStrand { int rid, off, len, K, cut_byte; bool rev; };
__device__ __forceinline__ FsStrand fs_strand(const mhip_offset_t* __restrict__ roffs, const ReadSel& sel, int ib, int s, bool cuts, int cut_step) {
    FsStrand d;
    d.rid = sel_rid(sel, ib + (s >> 1));
    d.off = roffs[d.rid].offset;
    d.len = roffs[d.rid].size;
    d.K = kmers_of(d.len);
    d.rev = s & 1;
    d.cut_byte = 7;                 // byte of the record's y:z that holds the bucket length for this read (seed_probe)
    if (cuts) {
        const long long need = (long long)d.off + d.len + 1 + 5 * ZV;
        const long long t = (need + cut_step - 1) / cut_step;
        if (t <= 7) d.cut_byte = (int)t - 1;
    }
    return d;
}
__device__ __forceinline__ int64_t fs_kmer_at(const FsStrand& d, int km) {
    return !d.rev ? (int64_t)d.off + (int64_t)km * BC : (int64_t)d.off + d.len - MHIP_KMER_SIZE - (int64_t)km * BC;
}
__device__ __forceinline__ void fs_hdr_words(const uint32_t* __restrict__ pac, const FsStrand& d, int km, uint32_t (&w)[2]) {
    const int64_t i = fs_kmer_at(d, km) >> 4;
    w[0] = pac[i];
    w[1] = pac[i + 1];
}
__device__ __forceinline__ void fs_hdr_record(const uint32_t* __restrict__ starts, const uint4* __restrict__ recs, const FsStrand& d, int km,
                                              const uint32_t (&w)[2], uint32_t (&r)[3]) {
    const uint64_t W = ((uint64_t)__builtin_bswap32(w[0]) << 32) | __builtin_bswap32(w[1]);      // pac_kmer
    uint32_t id = (uint32_t)(W >> (64 - 26 - (int)((fs_kmer_at(d, km) & 15) << 1))) & KMER_MASK;
    if (d.rev) id = kmer_revcomp(id);
    if (recs) {
        const uint4 v = recs[id];
        r[0] = v.x; r[1] = v.y; r[2] = v.z;
    } else {
        r[0] = starts[id]; r[1] = starts[id + 1];      // (r[2] is left alone: nothing here may touch a loaded value, see seed_strand)
    }
}
__device__ __forceinline__ void fs_hdr_decode(bool cuts, const FsStrand& d, const uint32_t (&r)[3], uint32_t* bs, uint32_t* cnt, uint32_t* all) {
    *bs = r[0];
    if (cuts) {
        // byte cut_byte of y:z, word by word (a 64-bit y:z here would make the compiler keep the raw records as one 64-bit value and
        // combine them where they are loaded: a wait behind the prefetch loads)
        *all = r[2] >> 24;
        *cnt = ((d.cut_byte < 4 ? r[1] : r[2]) >> (8 * (d.cut_byte & 3))) & 0xFFu;
    } else {
        *all = *cnt = r[1] - r[0];
    }
}

// ascending sort of p[0 .. n) (LDS, n <= 64 NQ) by one wave: bitonic network, element q * 64 + lane in register v[q]
template <int NQ>
__device__ __forceinline__ void fs_bitonic(uint32_t* p, const uint32_t n, const int lane) {
    uint32_t v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { const uint32_t idx = q * 64 + lane; v[q] = idx < n ? p[idx] : 0xFFFFFFFFu; }
#pragma unroll
    for (int k = 2; k <= NQ * 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= 64) {
                const int dq = j >> 6;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    if ((q & dq) == 0) {
                        const uint32_t a = v[q], b = v[q | dq];
                        const bool asc = ((q * 64) & k) == 0;         // k > j >= 64: the k bit of the index is a bit of q
                        v[q] = asc ? min(a, b) : max(a, b);
                        v[q | dq] = asc ? max(a, b) : min(a, b);
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const uint32_t o = (uint32_t)__builtin_amdgcn_ds_bpermute((lane ^ j) << 2, (int)v[q]);
                    const bool asc = (((q * 64 + lane) & k) == 0), lower = (lane & j) == 0;
                    v[q] = (asc == lower) ? min(v[q], o) : max(v[q], o);
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < NQ; ++q) { const uint32_t idx = q * 64 + lane; if (idx < n) p[idx] = v[q]; }
}

__device__ __forceinline__ uint32_t fs_cnt(const uint32_t* cnt32, uint32_t e) { return (cnt32[e >> 1] >> ((e & 1u) * 16u)) & 0xFFFFu; }

// seed_strand is persistent: one workgroup per CU, each taking strands from a cursor (ctl->next) one ahead of the strand it works on.
// The bucket headers of a strand (what seed_probe computes: start and size of the bucket of every query k-mer) are fetched by the
// workgroup itself and live in LDS for both walks, in the place of sq_id / sq_score, which the build writes only after walk 2.  Those
// of the NEXT strand are requested while the memory pipeline has nothing else to do: the packed words of the read in front of walk 2,
// the records behind it; the raw records (two per thread: K <= 2 * FS_THREADS) wait in registers through the LDS phases of this
// strand and are decoded at the top of the next.  Longer strands, the first strand of a workgroup and a strand behind one that left
// early fetch what is missing there, unhidden.  A strand with more than FS_SEGCAP k-mers is left to the kernel chain.
// A.km_bstart != nullptr (MECAT_SEED_FUSED_PROBE=0): seed_probe has run, the headers are copied from its arrays and nothing is tallied here.
// Registers.  A 1 024-thread workgroup may use 128 VGPRs per thread, and the kernel stands at that limit: 128 VGPRs, no scratch, 4 waves
// per SIMD (79 VGPRs before the strand loop: what LLVM hoists out of that loop — constants, lane masks — stays live through every phase).
// Several things here exist only to keep it out of scratch: the opaque thread index per strand, FS_UNI, the thread index handed to
// fs_walk / fs_excl_scan / fs_block_sum2, ds_bpermute with an explicit lane in place of __shfl_*, fs_bitonic inlined, the tallies in
// LDS.  After any edit to this kernel, and after a compiler change, check
//   hipcc --offload-arch=gfx950 <HIPFLAGS of the Makefile> -Rpass-analysis=kernel-resource-usage -c mecat_amd/csrc/seed_strand.hip
// for seed_strand: `ScratchSize [bytes/lane]: 0`, `VGPRs Spill: 0`, `Occupancy [waves/SIMD]: 4` (profiles/seed_headers.md has the record).
#define FS_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
__global__ __launch_bounds__(FS_THREADS) void seed_strand(const uint32_t* __restrict__ pac, const mhip_offset_t* __restrict__ roffs, ReadSel sel,
                                                          int ib, int ns, const uint32_t* __restrict__ starts, const uint4* __restrict__ recs,
                                                          int cut_step, const uint16_t* __restrict__ slots, const int32_t* __restrict__ offsets,
                                                          SeedArrays A, int gate, int hi_bits, int min_kmer_match, double cutoff,
                                                          unsigned long long cap, FusedCtl* __restrict__ ctl,
                                                          unsigned long long* __restrict__ counters, RefReads R) {
    __shared__ FsLds L;
    const int tid0 = threadIdx.x;
    const bool probed = A.km_bstart != nullptr;
    const bool cuts = recs != nullptr;
    uint32_t* const hbs = L.sq_id;                       // the strand's bucket headers, [K] (K <= FS_SEGCAP)
    uint16_t* const hcn = L.sq_score;
    constexpr int PF = 2;                                // prefetched records per thread
    uint32_t pw[PF][2], pr[PF][3];                       // the next strand's packed words / raw records of k-mers tid, tid + FS_THREADS
#pragma unroll
    for (int j = 0; j < PF; ++j) { pw[j][0] = pw[j][1] = 0; pr[j][0] = pr[j][1] = pr[j][2] = 0; }
    int pf = -1;                                         // the strand pr[] belongs to
    if (tid0 == 0) { L.tally[0] = L.tally[1] = L.tally[2] = 0; L.misc[8] = atomicAdd(&ctl->next, 1u); L.misc[9] = atomicAdd(&ctl->next, 1u); }
    __syncthreads();
    // (block-uniform values that decide a `continue` are made scalar: the strand loop then has uniform branches only)
    int s = (int)min(FS_UNI(L.misc[8]), (uint32_t)ns), sn = (int)min(FS_UNI(L.misc[9]), (uint32_t)ns), s2 = ns;
    for (; s < ns; s = sn, sn = s2) {
    __syncthreads();                                     // the strand before is through with the LDS (and everybody has read misc[8])
    // (the thread index is made opaque per strand: what is derived from it — addresses, masks — would otherwise be hoisted out of the strand
    // loop and held in registers across all phases, which costs the kernel its 4 waves per SIMD)
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FsStrand d = fs_strand(roffs, sel, ib, s, cuts, cut_step);
    const int rid = d.rid, rlen = d.len, K = d.K;
    auto fail = [&]() {                     // called by all threads together
        if (tid == 0) { A.fused[s] = 0; atomicAdd(&ctl->n_fallback, 1u); atomicAdd(&counters[14], 1ull); }      // debug slot 14: strands left to the kernel chain
    };
    unsigned long long t_prev = wall_clock64(); (void)t_prev;
    for (int i = tid; i < FLT_M / 2; i += FS_THREADS) L.x.cnt32[i] = 0;
    for (int i = tid; i < REL_WORDS; i += FS_THREADS) L.rel[i] = 0u;
    if (tid < 8) L.misc[tid] = 0;
    if (tid == 0) L.misc[8] = atomicAdd(&ctl->next, 1u);           // the strand after the next
    // ---- bucket headers -> LDS; hits of the strand
    uint32_t Hall, run_all;
    {
        const bool room = K <= FS_SEGCAP;                // (a longer strand fails below: only its sums are wanted)
        uint32_t hc = 0, ha = 0;
        if (probed) {
            const uint32_t kb = A.km_base[s];
            for (int km = tid; km < K; km += FS_THREADS) {
                const uint32_t bs = A.km_bstart[kb + km], cn = A.km_cnt[kb + km];
                hc += cn;
                if (room) { hbs[km] = bs; hcn[km] = (uint16_t)cn; }
            }
        } else {
            auto take = [&](int km, const uint32_t (&r)[3]) {
                uint32_t bs, cn, al;
                fs_hdr_decode(cuts, d, r, &bs, &cn, &al);
                hc += cn;
                ha += al;
                if (room) { hbs[km] = bs; hcn[km] = (uint16_t)cn; }
            };
            if (pf != s) {                               // nothing prefetched for this strand: its first records now
#pragma unroll
                for (int j = 0; j < PF; ++j)
                    if (tid + j * FS_THREADS < K) fs_hdr_words(pac, d, tid + j * FS_THREADS, pw[j]);
#pragma unroll
                for (int j = 0; j < PF; ++j)
                    if (tid + j * FS_THREADS < K) fs_hdr_record(starts, recs, d, tid + j * FS_THREADS, pw[j], pr[j]);
            }
            // (the first use of the raw records, pinned here: without it the compiler moves the word combine of fs_hdr_decode up to the
            // loads behind walk 2, and with it the wait for them)
#pragma unroll
            for (int j = 0; j < PF; ++j) asm volatile("" : "+v"(pr[j][0]), "+v"(pr[j][1]), "+v"(pr[j][2]));
#pragma unroll
            for (int j = 0; j < PF; ++j)
                if (tid + j * FS_THREADS < K) take(tid + j * FS_THREADS, pr[j]);
            for (int km = tid + PF * FS_THREADS; km < K; km += FS_THREADS) {
                uint32_t w[2], r[3] = {0, 0, 0};
                fs_hdr_words(pac, d, km, w);
                fs_hdr_record(starts, recs, d, km, w, r);
                take(km, r);
            }
        }
        fs_block_sum2(tid, hc, ha, L.red, &Hall, &run_all);   // (its barrier: the cleared tables, the headers and misc[8] are visible)
        Hall = FS_UNI(Hall);
        run_all = FS_UNI(run_all);
        s2 = (int)min(FS_UNI(L.misc[8]), (uint32_t)ns);
        if (!probed && tid == 0) { L.tally[0] += (unsigned long long)K; L.tally[1] += run_all; L.tally[2] += Hall; A.strand_hits_all[s] = Hall; }
    }
    if (Hall == 0) {
        if (tid == 0) { A.fused[s] = 1; A.strand_hits[s] = 0; A.hit_base[s] = 0; A.nseg[s] = 0; A.nrec[s] = 0; A.ngated[s] = 0; }
        continue;
    }
    // a 16-bit counter could wrap; km has 15 bits in the payload; the headers have FS_SEGCAP places
    if (Hall >= 65536u || K > 32767 || K > FS_SEGCAP) { fail(); continue; }

    // ---- walk 1: hits per table slot
    FS_MARK(0);
    fs_walk<FS_LPB1, FS_NP1, FS_Q1, FS_D1, false>(tid, hbs, hcn, slots, K, [&](int, uint32_t e) { atomicAdd(&L.x.cnt32[e >> 1], 1u << ((e & 1u) * 16u)); });
    __syncthreads();
    FS_MARK(1);

    // ---- relevance: hot slots, +- reach (seed_filter).  A thread owns one word of the bitmaps = 32 slots = 16 counter words,
    // which it keeps in registers from here to the region starts.
    static_assert(FLT_M / FS_THREADS == 32, "one bitmap word per thread");
    uint32_t cw[18];                   // cw[1 .. 16]: the thread's counters; cw[0], cw[17]: the neighbours' last / first word
    {
        const uint4* c4 = (const uint4*)&L.x.cnt32[16 * tid];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const uint4 v = c4[q]; cw[1 + 4 * q] = v.x; cw[2 + 4 * q] = v.y; cw[3 + 4 * q] = v.z; cw[4 + 4 * q] = v.w; }
        cw[0] = L.x.cnt32[(16 * tid - 1) & (FLT_M / 2 - 1)];
        cw[17] = L.x.cnt32[(16 * tid + 16) & (FLT_M / 2 - 1)];
        uint32_t hot = 0;
        {
#pragma unroll
        for (int j = 1; j <= 16; ++j) {
            const int lo = (int)(cw[j] & 0xFFFFu), hi = (int)(cw[j] >> 16), pl = (int)(cw[j - 1] >> 16), nx = (int)(cw[j + 1] & 0xFFFFu);
            const bool hl = lo > 0 && (lo + hi >= gate || lo + pl >= gate);
            const bool hh = hi > 0 && (hi + nx >= gate || hi + lo >= gate);
            hot |= (hl ? 1u : 0u) << (2 * (j - 1)) | (hh ? 1u : 0u) << (2 * (j - 1) + 1);
        }
        const uint32_t reach = (uint32_t)min(sweep_reach(rlen), FLT_M / 2 - 1);
        for (uint32_t m = hot; m; m &= m - 1u) {
            const uint32_t e = (uint32_t)tid * 32u + (uint32_t)__builtin_ctz(m);
            uint32_t lo = (e - reach) & (FLT_M - 1), left = 2 * reach + 1;
            while (left > 0) {
                const uint32_t b = lo & 31u, take = min(32u - b, left);
                const uint32_t msk = (take == 32u ? 0xFFFFFFFFu : ((1u << take) - 1u)) << b;
                atomicOr(&L.rel[lo >> 5], msk);
                lo = (lo + take) & (FLT_M - 1);
                left -= take;
            }
        }
        }
    }
    __syncthreads();
    FS_MARK(2);
    // ---- occupied relevant slots, region starts
    uint32_t kept;
    {
        const uint32_t r = L.rel[tid];
        uint32_t occ = 0, mine = 0;
        bool toolong = false;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const uint32_t h = (cw[1 + (j >> 1)] >> ((j & 1) * 16)) & 0xFFFFu;
            if (((r >> j) & 1u) && h) { occ |= 1u << j; mine += h; toolong |= h > FS_BIGN; }
        }
        // one scan for both prefixes: hits in the low half (Hall < 2^16), occupied slots in the high half (<= 2^15)
        uint32_t both;
        const uint32_t exb = fs_excl_scan(tid, mine | ((uint32_t)__popc(occ) << 16), L.wtot, &both);
        const uint32_t ex = exb & 0xFFFFu, cx = exb >> 16;
        kept = FS_UNI(both) & 0xFFFFu;
        if (kept > FS_CAP) { fail(); continue; }
        L.occ[tid] = occ;
        L.base_ci[tid] = (uint16_t)cx;
        uint16_t* cur16 = (uint16_t*)L.y.cur32;
        uint32_t at = ex, ci = cx;
        if (occ) {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const uint32_t h = (cw[1 + (j >> 1)] >> ((j & 1) * 16)) & 0xFFFFu;
                if ((occ >> j) & 1u) { cur16[ci++] = (uint16_t)at; at += h; }
            }
        }
        if (toolong) L.misc[3] = 1;
        __syncthreads();
        if (FS_UNI(L.misc[3])) { fail(); continue; }
    }
    if (kept == 0) {
        if (tid == 0) { A.fused[s] = 1; A.strand_hits[s] = 0; A.hit_base[s] = 0; A.nseg[s] = 0; A.nrec[s] = 0; A.ngated[s] = 0; }
        continue;
    }
    // room in the shared output arrays
    if (tid == 0) {
        const unsigned long long hb0 = atomicAdd(&ctl->alloc, (unsigned long long)kept);
        if (hb0 + kept > cap) L.misc[3] = 1;
        L.misc[6] = (uint32_t)hb0;
        L.misc[7] = (uint32_t)(hb0 >> 32);
    }
    __syncthreads();                                      // also: cnt32 is dead from here, the payload arrays take its place
    if (FS_UNI(L.misc[3])) { fail(); continue; }
    const uint64_t hb = ((uint64_t)L.misc[7] << 32) | L.misc[6];

    FS_MARK(3);
    // ---- the next strand's headers, step 1: the packed words of its k-mers (they arrive during walk 2)
    const bool ahead = !probed && sn < ns;
    FsStrand dn = d;
    if (ahead) {
        dn = fs_strand(roffs, sel, ib, sn, cuts, cut_step);
#pragma unroll
        for (int j = 0; j < PF; ++j)
            if (tid + j * FS_THREADS < dn.K) fs_hdr_words(pac, dn, tid + j * FS_THREADS, pw[j]);
    }
    // ---- walk 2: kept hits into their slot's region
    // A kept hit is rare (one in nine): the wave parks kept hits in its queue and places 64 of them at a time, so that the
    // cursor arithmetic runs with every lane busy.
    {
        uint32_t qn = 0;                                  // wave-uniform: hits in this wave's queue
        auto place = [&](uint32_t qi) {
            const uint32_t pos = L.qpos[wv][qi], km = L.qkm[wv][qi];
            const uint32_t seg = pos / (uint32_t)ZV, off = pos - seg * (uint32_t)ZV;
            const uint32_t e = seg & (FLT_M - 1), w = e >> 5, b = e & 31u;
            const uint32_t oc = L.occ[w];
            const uint32_t ci = (uint32_t)L.base_ci[w] + (uint32_t)__popc(oc & ((1u << b) - 1u));
            const uint32_t sh = (ci & 1u) * 16u;
            const uint32_t p = (atomicAdd(&L.y.cur32[ci >> 1], 1u << sh) >> sh) & 0xFFFFu;
            L.x.e.pay[p] = ((seg >> FLT_BITS) << 26) | (km << 11) | off;
            L.x.e.eslot[p] = (uint16_t)e;
        };
        fs_walk<FS_LPB2, FS_NP2, FS_Q2, FS_D2, true>(tid, hbs, hcn, offsets, K, [&](int km, uint32_t pos, bool valid) {
            const uint32_t seg = pos / (uint32_t)ZV;
            const uint32_t e = seg & (FLT_M - 1);
            const uint32_t oc = valid ? L.occ[e >> 5] : 0u;
            const bool keep = (bool)((oc >> (e & 31u)) & 1u);
            const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
            if (m) {
                if (keep) {
                    const uint32_t at = qn + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    L.qpos[wv][at] = pos;
                    L.qkm[wv][at] = (uint16_t)km;
                }
                qn += (uint32_t)__popcll(m);
                if (qn >= 64u) { qn -= 64u; place(qn + (uint32_t)lane); }
            }
        });
        if ((uint32_t)lane < qn) place((uint32_t)lane);
    }
    // ---- the next strand's headers, step 2: the records.  The memory pipeline is idle from here to the output of this strand, and
    // nothing waits for these loads before the top of the next iteration (unless this strand's own few loads and stores do: vmcnt
    // counts in order, and by then the records have long arrived).
    if (ahead) {
#pragma unroll
        for (int j = 0; j < PF; ++j)
            if (tid + j * FS_THREADS < dn.K) fs_hdr_record(starts, recs, dn, tid + j * FS_THREADS, pw[j], pr[j]);
        pf = sn;
    }
    __syncthreads();
    FS_MARK(4);
    // ---- region sort.  After walk 2 cursor[ci] = end of region ci = start of region ci + 1.
    {
        const uint16_t* cur16 = (const uint16_t*)L.y.cur32;
        // short regions: every element counts the smaller elements of its region (all reads, barrier, all writes)
        uint32_t val[FS_CAP / FS_THREADS], dst[FS_CAP / FS_THREADS];
#pragma unroll
        for (int rd = 0; rd < FS_CAP / FS_THREADS; ++rd) {
            const uint32_t i = (uint32_t)rd * FS_THREADS + tid;
            dst[rd] = 0xFFFFFFFFu;
            val[rd] = 0;
            if ((uint32_t)rd * FS_THREADS < kept && i < kept) {
                const uint32_t v = L.x.e.pay[i], e = L.x.e.eslot[i], w = e >> 5, oc = L.occ[w];
                const uint32_t ci = (uint32_t)L.base_ci[w] + (uint32_t)__popc(oc & ((1u << (e & 31u)) - 1u));
                const uint32_t st = ci ? cur16[ci - 1] : 0u, en = cur16[ci], n = en - st;
                if (n > FS_SMALLN) {
                    if (i == st) L.x.e.big[atomicAdd(&L.misc[0], 1u)] = (uint16_t)ci;
                } else if (n > 1) {
                    uint32_t rank = 0;
                    for (uint32_t k = st; k < en; ++k) rank += L.x.e.pay[k] < v ? 1u : 0u;
                    val[rd] = v;
                    dst[rd] = st + rank;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int rd = 0; rd < FS_CAP / FS_THREADS; ++rd)
            if (dst[rd] != 0xFFFFFFFFu) L.x.e.pay[dst[rd]] = val[rd];
        FS_MARK(11);
        // long regions (a read meeting itself: ~200 hits per segment): one wave each, bitonic network in registers
        const uint32_t nbig = L.misc[0];
        for (uint32_t k = wv; k < nbig; k += FS_WAVES) {
            const uint32_t ci = L.x.e.big[k];
            const uint32_t st = ci ? cur16[ci - 1] : 0u, n = (uint32_t)cur16[ci] - st;      // FS_SMALLN < n <= FS_BIGN
            if (n <= 64) fs_bitonic<1>(L.x.e.pay + st, n, lane);
            else if (n <= 256) fs_bitonic<4>(L.x.e.pay + st, n, lane);
            else fs_bitonic<8>(L.x.e.pay + st, n, lane);
        }
        __syncthreads();
    }

    FS_MARK(5);
    // ---- build, phase A: recorded events (first hit of each (segment, km)) and segment heads, events compacted in place.
    // A thread takes a run of consecutive elements into registers; one scan; then everybody writes.
    uint32_t nrec, nseg;
    {
        constexpr int CHMAX = FS_CAP / FS_THREADS;
        const uint32_t ch = (kept + FS_THREADS - 1) / FS_THREADS;
        const uint32_t i0 = (uint32_t)tid * ch;
        uint32_t pv[CHMAX], sv[CHMAX];
        uint32_t ppay = 0, psl = 0xFFFFFFFFu;                       // no element before the first: a head
        if (i0 > 0 && i0 < kept) { ppay = L.x.e.pay[i0 - 1]; psl = L.x.e.eslot[i0 - 1]; }
        uint32_t hm = 0, rm = 0;
#pragma unroll
        for (int c = 0; c < CHMAX; ++c) {
            const uint32_t i = i0 + c;
            const bool in = (uint32_t)c < ch && i < kept;
            pv[c] = in ? L.x.e.pay[i] : 0u;
            sv[c] = in ? L.x.e.eslot[i] : 0u;
            const bool head = in && (sv[c] != psl || (pv[c] >> 26) != (ppay >> 26));
            const bool rec = in && (head || ((pv[c] >> 11) & 0x7FFFu) != ((ppay >> 11) & 0x7FFFu));
            hm |= (head ? 1u : 0u) << c;
            rm |= (rec ? 1u : 0u) << c;
            if (in) { ppay = pv[c]; psl = sv[c]; }
        }
        uint32_t both;
        const uint32_t ex = fs_excl_scan(tid, (uint32_t)__popc(rm) | ((uint32_t)__popc(hm) << 16), L.wtot, &both);     // its barriers come after all the reads
        uint32_t rpos = ex & 0xFFFFu, spos = ex >> 16;
        both = FS_UNI(both);
        nrec = both & 0xFFFFu;
        nseg = both >> 16;
        if (nseg > FS_SEGCAP) { fail(); continue; }
#pragma unroll
        for (int c = 0; c < CHMAX; ++c) {
            if ((rm >> c) & 1u) {
                if ((hm >> c) & 1u) {
                    L.sq_id[spos] = ((pv[c] >> 26) << FLT_BITS) | sv[c];
                    L.sq_st[spos] = (uint16_t)rpos;
                    ++spos;
                }
                L.x.e.pay[rpos++] = ((pv[c] & 0x7FFu) << 16) | ((((pv[c] >> 11) & 0x7FFFu) + 1u) & 0xFFFFu);
            }
        }
        if (tid == 0) L.sq_st[nseg] = (uint16_t)nrec;
    }
    uint16_t* perm = L.y.perm;                           // the cursors are dead
    __syncthreads();

    FS_MARK(6);
    // ---- segment order: stable split of the slot-major table on the segment bits above the slot bits
    if (hi_bits == 0) {
        for (uint32_t q = tid; q < nseg; q += FS_THREADS) perm[q] = (uint16_t)q;
    } else {
        uint32_t* hist = &L.x.e.hist[0][0];
        hist[tid] = 0;                                    // FS_WAVES * 64 == FS_THREADS
        __syncthreads();
        const uint32_t chunk = (((nseg + FS_WAVES - 1) / FS_WAVES) + 63u) & ~63u;
        const uint32_t lo = min(nseg, (uint32_t)wv * chunk), hi = min(nseg, lo + chunk);
        for (uint32_t q = lo + lane; q < hi; q += 64) atomicAdd(&L.x.e.hist[wv][L.sq_id[q] >> FLT_BITS], 1u);
        __syncthreads();
        {
            const uint32_t bin = tid >> 4, w = tid & 15;         // (bin major, wave minor)
            static_assert(FS_WAVES == 16, "16 waves");
            const uint32_t v = L.x.e.hist[w][bin];
            uint32_t all;
            const uint32_t ex = fs_excl_scan(tid, v, L.wtot, &all);
            L.x.e.hist[w][bin] = ex;
        }
        __syncthreads();
        volatile uint32_t* cur = L.x.e.hist[wv];
        const uint64_t lt = (1ull << lane) - 1ull;
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            const uint32_t q = q0 + lane;
            const bool valid = q < hi;
            const uint32_t d = valid ? L.sq_id[q] >> FLT_BITS : 0u;
            uint64_t peers = __ballot(valid);
            for (int b = 0; b < hi_bits; ++b) {
                const uint64_t m = __ballot((d >> b) & 1u);
                peers &= ((d >> b) & 1u) ? m : ~m;
            }
            const uint32_t rank = __popcll(peers & lt);
            const uint32_t base = valid ? cur[d] : 0u;
            if (valid) perm[base + rank] = (uint16_t)q;
            if (valid && rank == 0) cur[d] = base + (uint32_t)__popcll(peers);
        }
    }
    FS_MARK(7);
    // ---- phase B: scores; overflowed segments
    uint16_t* ovf = L.x.e.big;
    for (uint32_t q = tid; q < nseg; q += FS_THREADS) {
        const uint32_t c = (uint32_t)L.sq_st[q + 1] - (uint32_t)L.sq_st[q];
        if (c > SM) {
            const uint32_t k = atomicAdd(&L.misc[1], 1u);
            if (k < FS_BIGCAP) ovf[k] = (uint16_t)q;
            L.sq_score[q] = (uint16_t)FS_OVF16;
        } else {
            L.sq_score[q] = (uint16_t)c;
        }
    }
    __syncthreads();
    if (FS_UNI(L.misc[1]) > FS_BIGCAP) { fail(); continue; }
    // ---- phase C: insert_loc replay, one wave per overflowed segment (final lists and running scores go to HBM)
    {
        const uint32_t novf = L.misc[1];
        for (uint32_t k = wv; k < novf; k += FS_WAVES) {
            const uint32_t q = ovf[k];
            const uint32_t st = L.sq_st[q], en = L.sq_st[q + 1];
            int sc;
            replay_overflow(L.x.e.pay + st, (int)(en - st), A.ent_fin + hb + st, A.escore + hb + st, cutoff, &sc);
            if (lane == 0) L.sq_score[q] = (uint16_t)((uint32_t)sc | FS_OVF16);
        }
    }
    __syncthreads();
    FS_MARK(8);
    // ---- phase D: index_score and the gate, in segment order
    for (uint32_t g = tid; g < nseg; g += FS_THREADS) {
        const uint32_t q = perm[g];
        const uint32_t sid = L.sq_id[q];
        int s_k = (int)(L.sq_score[q] & 0x7FFFu);
        if (g > 0 && sid > 0) {
            const uint32_t ql = perm[g - 1];
            if (L.sq_id[ql] == sid - 1u) {
                const uint32_t st = L.sq_st[ql], en = L.sq_st[ql + 1];
                const uint32_t t = L.x.e.pay[(uint32_t)L.sq_st[q + 1] - 1u] & 0xFFFFu;       // km + 1 of this segment's last event
                uint32_t lo = st, hi = en;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if ((L.x.e.pay[mid] & 0xFFFFu) <= t) lo = mid + 1; else hi = mid;
                }
                if (lo > st) s_k += (L.sq_score[ql] & FS_OVF16) ? (int)A.escore[hb + lo - 1] : (int)(lo - st);
            }
        }
        bool listed = (int)(int16_t)s_k >= 2 * min_kmer_match;
        if (listed && R.enable) listed = !subjects_all_higher(R, sid, rid, roffs[rid].offset + rlen + 1);
        if (listed) {
            const uint32_t k = atomicAdd(&L.misc[2], 1u);
            if (k < FS_GATECAP) {
                const uint32_t e0 = L.x.e.pay[L.sq_st[q]];
                L.gate[k] = (uint16_t)g;
                L.x.e.tf[k] = ((uint64_t)((e0 & 0xFFFFu) - 1u) << 32) | (uint64_t)(sid * (uint32_t)ZV + (e0 >> 16));
            }
        }
    }
    __syncthreads();
    const uint32_t ng = FS_UNI(L.misc[2]);
    if (ng > FS_GATECAP) { fail(); continue; }
    FS_MARK(9);
    // ---- phase E + output
    for (uint32_t a = tid; a < ng; a += FS_THREADS) {
        const uint64_t ta = L.x.e.tf[a];
        uint32_t rank = 0;
        for (uint32_t b = 0; b < ng; ++b) rank += L.x.e.tf[b] < ta ? 1u : 0u;
        A.gated[hb + rank] = (uint32_t)L.gate[a];
    }
    for (uint32_t i = tid; i < nrec; i += FS_THREADS) A.ent[hb + i] = L.x.e.pay[i];
    for (uint32_t g = tid; g < nseg; g += FS_THREADS) {
        const uint32_t q = perm[g];
        const uint32_t sc = L.sq_score[q];
        A.seg_id[hb + g] = L.sq_id[q];
        A.seg_start[hb + g] = L.sq_st[q];
        A.seg_score[hb + g] = (int32_t)((sc & 0x7FFFu) | ((sc & FS_OVF16) ? OVF_FLAG : 0u));
    }
    FS_MARK(10);
    if (tid == 0) {
        atomicAdd(&counters[13], 1ull);                   // debug slot 13: strands that went through this kernel with hits
        A.fused[s] = 1;
        A.strand_hits[s] = kept;
        A.hit_base[s] = hb;
        A.nseg[s] = nseg;
        A.nrec[s] = nrec;
        A.ngated[s] = ng;
    }
    }       // strands
    if (!probed && tid0 == 0) {              // what seed_probe tallies, once per workgroup
        atomicAdd(&counters[0], L.tally[0]);
        atomicAdd(&counters[1], L.tally[1]);
        if (cuts) atomicAdd(&counters[15], L.tally[2]);      // debug slot 15: bucket hits walked with the cuts on
    }
}

#undef FS_UNI

// ------------------------------------------------------------------------------------------------ launcher
// development (tools/dev/seed_stats.py): per-strand sizes of the strand pipeline
static int print_strand_stats(const SeedBatch& b) {
    const int ns = b.ns;
    std::vector<uint32_t> h[5];
    const uint32_t* src[5] = {b.A.strand_hits_all, b.F.strand_hits, b.F.nseg, b.F.nrec, b.F.ngated};
    for (int i = 0; i < 5; ++i) { h[i].resize((size_t)ns); HIPCHK(hipMemcpy(h[i].data(), src[i], sizeof(uint32_t) * (size_t)ns, hipMemcpyDeviceToHost)); }
    std::vector<int32_t> fu((size_t)ns);
    HIPCHK(hipMemcpy(fu.data(), b.A.fused, sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost));
    for (int s = 0; s < ns; ++s)
        if (fu[(size_t)s]) fprintf(stderr, "SEEDSTAT %d %u %u %u %u %u\n", s & 1, h[0][(size_t)s], h[1][(size_t)s], h[2][(size_t)s], h[3][(size_t)s], h[4][(size_t)s]);
    return 0;
}

// Tables of the strands seed_strand takes, in arrays handed out by an atomic cursor.  The host waits for FusedCtl (the first of a
// batch's two waits): *n_fallback strands are left to the kernel chain.
// (PacBio gates only.  A form of this kernel behind seed_filter_wide, for the low gates of nanopore mode, was built in round 5 and measured
// slower than the chain it replaced — 59.4 ms against seed_emit 26.6 + seed_sort_pass 13.7 + seed_build 8.6 = 48.9 ms on 100 000 ONT-style
// reads of 20 kb, its second bucket walk costing more than the two sort passes and the build it saved — and was removed in round 6.)
int seed_run_strand(SeedBatch& b, unsigned int* n_fallback) {
    mhip_ctx* c = b.c;
    SeedArrays& F = b.F;
    const int ns = b.ns;
    // room: the relevance filter keeps about one bucket hit in nine; a strand that finds the arrays full takes the kernel chain
    size_t capF = (size_t)((double)b.sumK * b.hits_per_lookup / 5.0) + (size_t)ns * 256 + 64;
    if (b.knobs.fused_room > 0) capF = (size_t)b.knobs.fused_room;      // test knob: entries in the shared arrays
    FusedCtl* d_ctl;
    if (c->scratch("sf_ctl", sizeof(FusedCtl), (void**)&d_ctl)) return -1;
    if (seed_strand_tables(c, "sf_", ns, &F)) return -1;
    if (seed_hit_tables(c, "sf_", capF, &F)) return -1;
    HIPCHK(hipMemsetAsync(d_ctl, 0, sizeof(FusedCtl), c->stream));
    // one workgroup per CU (its LDS holds one strand); the workgroups take the strands from a cursor in *d_ctl
    LAUNCH(c, "seed_strand", seed_strand, std::min(ns, std::max(1, c->num_cus)), FS_THREADS, 0, (const uint32_t*)b.reads->d_pac,
           (const mhip_offset_t*)b.reads->d_offs, b.sel, b.ib, ns, (const uint32_t*)b.idx->d_starts, b.recs, b.cut_step,
           (const uint16_t*)b.idx->d_slots, (const int32_t*)b.idx->d_offsets, F, b.gate, std::max(0, b.nbits - FLT_BITS), (int)b.P->min_kmer_match,
           b.P->ddfs_cutoff, (unsigned long long)capF, d_ctl, (unsigned long long*)c->d_counters, b.RR);
    FusedCtl ctl;
    HIPCHK(hipMemcpyAsync(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_fallback = ctl.n_fallback;
#ifdef FS_PROF
    for (int i = 0; i < 12; ++i) fprintf(stderr, "FS_PROF phase %d: F %.1f R %.1f us per strand\n", i, (double)ctl.prof[i] / 50.0 / ns, (double)ctl.prof[i + 16] / 50.0 / ns);
#endif
    if (getenv("MECAT_SEED_STATS")) return print_strand_stats(b);
    return 0;
}
