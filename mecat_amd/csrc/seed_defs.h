// seed_defs.h — what the host side of the seeding stage (seed.hip) and every kernel family share: the sizes, the batch arrays, the
// read selection, the key and entry formats, and the description of one batch that the three families' launchers take.
//   seed_chain.hip   seed_probe, seed_scan, seed_filter, seed_filter_wide, seed_emit, seed_sort_pass, seed_build
//   seed_strand.hip  seed_strand
//   seed_cand.hip    seed_cand
// Device helpers that more than one family calls are in seed_replay.h and seed_walk.h.
#pragma once

#include "common.h"

#define SEED_BLOCK 256
#define SEED_WAVES (SEED_BLOCK / WAVE)
#define KEY_OFF_BITS 11
#define KEY_KM_BITS 16
#define KEY_SEG_SHIFT (KEY_OFF_BITS + KEY_KM_BITS)   // 27
#define MAXC_LDS 1024                 // top-MAXC lists up to this size live in LDS; longer ones in the output array itself
#define MAXC_LIMIT (1 << 20)
#define FLT_BITS 15                 // relevance filter: 2^15 8-bit hit counters per strand, segment ids hashed by their low bits
#define FLT_M (1 << FLT_BITS)
#define REL_WORDS (FLT_M / 32)      // relevance bitmap over the same hashed ids

struct SeedArrays {
    // per batch
    const uint32_t* km_base;     // [ns]   first k-mer slot of the strand
    uint32_t* km_bstart;         // [sumK] bucket start in index offsets[]
    uint32_t* km_cnt;            // [sumK] bucket size
    uint32_t* strand_hits_all;   // [ns]   bucket hits of the strand (before the relevance filter)
    uint32_t* strand_hits;       // [ns]   hits kept (emitted, sorted, built)
    uint32_t* rel_bits;          // [ns * REL_WORDS] relevance bitmap of the strand (filtered strands only)
    int32_t* filtered;           // [ns]   1 = only relevant hits are kept, 0 = every hit is kept
    int32_t* fused;              // [ns]   1 = the strand went through seed_strand (its tables live in the fused arrays)
    uint32_t rel_mask;           // relevance bitmap bit of segment seg: ((seg & rel_mask) >> rel_shift): 2^15 - 1 and 0 for seed_filter,
    uint32_t rel_shift;          //   2^18 - 1 and 3 for seed_filter_wide
    uint64_t* hit_base;          // [ns + 1]
    uint64_t* keysA;             // [Htot]
    uint64_t* keysB;             // [Htot]
    uint32_t* ent;               // [Htot] recorded events: off << 16 | (uint16)(km + 1)
    uint32_t* ent_fin;           // [Htot] final 40-entry lists of overflowed segments (same indexing as ent)
    uint16_t* escore;            // [Htot] score after each recorded event (overflowed segments only)
    uint32_t* seg_id;            // [Htot] segment table, ascending seg id
    uint32_t* seg_start;         // [Htot] first recorded event of the segment in ent[]
    int32_t* seg_score;          // [Htot] live Back_List.score (bit 30 set: lists live in ent_fin)
    uint32_t* seg_kmlast;        // [Htot] km of the segment's last recorded event
    uint64_t* seg_tfirst;        // [Htot] first-touch time (km << 32 | position)
    uint32_t* gated;             // [Htot] segment-table indices passing the index_score gate, in first-touch order
    uint32_t* nseg;              // [ns]
    uint32_t* nrec;              // [ns]
    uint32_t* ngated;            // [ns]
};

#define OVF_FLAG 0x40000000

__host__ __device__ __forceinline__ int kmers_of(int L) { return L < MHIP_KMER_SIZE ? 0 : (L - MHIP_KMER_SIZE) / BC + 1; }

// Which reads a call works on: local index i -> read rid0 + (i / chunk) * cstride + i % chunk.  chunk == 1 is a plain stride
// (a contiguous range has cstride == 1); chunk > 1 is the multi-GPU shard of a grid cell by chunks of reads (SURVEY.md §8e:
// the reference hands out chunks of 500 reads, mecat2pw/pw_impl.cpp:612-621; rank r of P owns every P-th chunk).
struct ReadSel { int rid0, chunk, cstride; };
__host__ __device__ __forceinline__ int sel_rid(const ReadSel& s, int i) {
    return s.chunk == 1 ? s.rid0 + i * s.cstride : s.rid0 + (i / s.chunk) * s.cstride + i % s.chunk;
}

// a key (keysA / keysB) is seg:21 | km:16 | off:11; a recorded event (ent / ent_fin) is off << 16 | (uint16)(km + 1)
__device__ __forceinline__ uint32_t key_seg(uint64_t k) { return (uint32_t)(k >> KEY_SEG_SHIFT); }
__device__ __forceinline__ uint32_t key_km(uint64_t k) { return (uint32_t)(k >> KEY_OFF_BITS) & 0xFFFFu; }
__device__ __forceinline__ uint32_t key_off(uint64_t k) { return (uint32_t)k & 0x7FFu; }
__device__ __forceinline__ int ent_loc(uint32_t e) { return (int)(e >> 16); }
__device__ __forceinline__ int ent_seed(uint32_t e) { return (int)(int16_t)(e & 0xFFFFu); }

// what the segment builders need to know about the reference volume: a gated segment whose every possible subject read has a
// higher id than the query read is not listed (get_candidates would vote on it and then drop it at `sid > read_id`,
// pw_impl.cpp:370, before anything is written: half of the gated segments of a diagonal grid cell)
struct RefReads { const mhip_offset_t* offs; const uint32_t* blk; int nreads, start_id, reads_start_id, enable, same_volume; };

// ------------------------------------------------------------------------------------------------ one batch, host side
// the debug and tuning knobs: read from the environment and the parameters at the top of every call (seed.hip: read_knobs), never cached
struct SeedKnobs {
    bool filter;          // relevance filter of seed_filter / seed_strand: 2 * min_kmer_match >= 6 and MECAT_SEED_FILTER is not 0
    bool wide_filter;     // seed_filter_wide: the gate in [4, 6) and the same knob
    bool fused;           // the strand pipeline: the filter is on and MECAT_SEED_FUSED is not 0
    bool fused_probe;     // seed_strand fetches its bucket headers itself: MECAT_SEED_FUSED_PROBE is not 0
    bool cuts;            // buckets of a diagonal cell cut behind the read's own copy: MECAT_SEED_CUTS is not 0
    bool predrop;         // gated segments with higher subjects only are not listed: MECAT_SEED_PREDROP is not 0
    double fused_room;    // MECAT_SEED_FUSED_ROOM: entries in seed_strand's shared arrays, 64 at least; 0 = not set, sized from the batch
    double batch_hits;    // MECAT_SEED_BATCH_HITS: estimated bucket hits per batch, 1e6 at least; 0 = not set, the rule of next_batch_end
};

// One batch = the reads with local index [ib, ib + nr) of the selection.  Filled once (seed.hip: plan_batch), then handed from step to
// step of seed_batch.  A holds what is common to both formulations; F and B start as copies of it and get the tables of the strands
// seed_strand built (F, scratch "sf_*") and of those the kernel chain built (B, scratch "sd_*"); seed_cand reads both.
struct SeedBatch {
    mhip_ctx* c;
    const mhip_index* idx;
    const mhip_volume *ref, *reads;
    ReadSel sel;
    int ib, nr, ns;               // ns = 2 nr strands
    uint64_t sumK;                // k-mers of all strands
    const mhip_params* P;
    mhip_candidate* d_out;        // [nr * maxc]
    int32_t* d_counts;            // [nr]
    const uint4* recs;            // the index's cut records on a diagonal cell with the cuts on, else nullptr
    int cut_step;
    int gate;                     // 2 * min_kmer_match
    int nbits;                    // bits of a segment id of the reference volume
    RefReads RR;
    SeedKnobs knobs;
    double hits_per_lookup;
    SeedArrays A, F, B;
    std::vector<uint32_t> kmb;    // [ns] host copy of km_base: the source of an async upload, alive until seed_batch returns
};

// the tables both formulations hand to seed_cand, from scratch buffers named prefix ("sf_" or "sd_") + table: one entry per strand ...
int seed_strand_tables(mhip_ctx* c, const char* prefix, int ns, SeedArrays* T);
// ... and one per kept hit
int seed_hit_tables(mhip_ctx* c, const char* prefix, size_t cap, SeedArrays* T);

// The launchers, each beside its kernels.  All work on the context's stream; the two host waits of a batch are in seed_run_strand (for
// FusedCtl) and in seed_run_chain (for the number of kept hits).
int seed_run_probe(SeedBatch& b, int tally);                     // seed_chain.hip: bucket headers of every strand -> A.km_bstart, A.km_cnt
int seed_run_strand(SeedBatch& b, unsigned int* n_fallback);     // seed_strand.hip: fills F; -> strands left to the chain
int seed_run_chain(SeedBatch& b);                                // seed_chain.hip: fills B for the strands with fused[s] == 0
int seed_run_cand(const SeedBatch& b);                           // seed_cand.hip
