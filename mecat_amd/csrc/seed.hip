// seed.hip — host side of the seeding stage: k-mer probe, DDF block-scoring seed filter and candidate selection.
//
// Replaces, for a batch of query reads and both strands of each:
//   extract_kmers      mecat2pw/pw_impl.cpp:83-97      query k-mers at stride 10
//   seeding            mecat2pw/pw_impl.cpp:241-286    bucket walk, per-2kb-segment seed lists (Back_List), index_score
//   insert_loc         mecat2pw/pw_impl.cpp:121-159    >40-seeds-per-segment overflow policy
//   find_location      mecat2pw/pw_impl.cpp:161-239    DDF vote inside a segment pair
//   get_candidates     mecat2pw/pw_impl.cpp:288-465    gate, subject lookup, self-hit scrub, neighbour sweeps, top-MAXC
//
// The reference keeps a 168-byte Back_List per 2 kb of reference per thread (126 MB at 1.5 Gbase) and updates it in
// hit order.  That state is order dependent (SURVEY.md §7 "hard parts" 1-3), so the GPU formulation is a replay: ascending
// (segment, query k-mer, position) is the order the reference visits the hits of a segment in.  Two formulations build the tables of
// a strand (recorded events, segment table, gated segments in first-touch order), and seed_cand reads either, strand by strand:
//
// The strand pipeline (seed_strand.hip), PacBio gates only (2 * min_kmer_match >= 6, relevance filter on, MECAT_SEED_FUSED not 0):
//   seed_strand (1 024 threads / CU, persistent)  takes strands from a cursor and owns a strand from the bucket headers to the segment
//                                 table; the kept hits stay in LDS.  A strand that does not fit (k-mers, bucket hits, kept hits, segments, a slot
//                                 piled too high, the shared output arrays full) is left to the kernel chain: fused[s] stays 0
//
// The kernel chain (seed_chain.hip), for every strand seed_strand left or, with the pipeline off (nanopore gates, knobs), for all:
//   seed_probe  (block / strand)  2-bit read -> 13-mers (reverse strand by index arithmetic) -> bucket (start, count) from the
//                                 starts[] table or, on a diagonal cell, the cut records; hits per strand.  Runs for the whole batch:
//                                 first when the pipeline is off or MECAT_SEED_FUSED_PROBE=0 (seed_strand then copies its headers),
//                                 else behind seed_strand and only when a strand was left, without tallying the lookups again
//   seed_filter (block / strand)  relevance filter at gates >= 6: one walk over the buckets counts hits per (hashed) 2 kb segment in
//                                 LDS; segments that can reach the index_score gate, +- the sweep reach, form the relevance
//                                 bitmap; every other hit (6 of 7 at config 2) is never expanded.  With the filter off
//                                 (MECAT_SEED_FILTER=0, or a gate below 4) it only passes the hit counts on: every hit is kept
//   seed_filter_wide (1 024 threads / strand)  gates in [4, 6), nanopore mode: the same with 2^18 slots and 4-bit counters in the LDS of a CU
//   seed_scan   (one block)       exclusive scan of kept hits per strand -> region of every strand in the batch arrays
//   seed_emit   (block / strand)  expand the kept hits: key = seg:21 | km:16 | off:11 written in (km, position) order,
//                                 i.e. in the order the reference visits the hits (64 buckets per step: count, scan, write)
//   seed_sort_pass (block / strand)  stable LSD radix sort on the seg bits only (up to SORT_MAXBITS = 11 bits per pass, two passes for
//                                 the 20-21 segment bits of a full volume): ranking by wave64 ballot multi-split, per-wave cursors in
//                                 LDS, no atomics in the scatter loop.  Stability keeps (km, position) order inside a segment
//   seed_build  (block / strand)  "recorded" events = first hit of each (segment, km) (pw_impl.cpp:265,282);
//                                 ballot/prefix compaction into per-segment seed lists; segments with > 40 recorded
//                                 events replay insert_loc one wave per segment (exact-diagonal fast path for the
//                                 read hitting itself); index_score incl. the left neighbour's score at the time of
//                                 the segment's last event; gated segments ordered by first-touch time
//
// Candidates (seed_cand.hip):
//   seed_cand   (wave / read)     sequential replay of get_candidates over the gated segments of F then R strand:
//                                 lanes evaluate the O(n^2) DDF votes, the sweeps and the list shifts in parallel
//
// FP: find_location is all f32, insert_loc divides in f32 and compares in f64, the sweeps are f64;
// built with -ffp-contract=off and hipcc's default correctly-rounded f32 division.
//
// Reads longer than 327 670 bases: the reference's seed numbers are `short` and wrap.  ent_seed() sign-extends the stored 16
// bits like the reference's loads do, the recording rule follows the wrapped `seednum` (seed_build, phase A), and such a strand always takes the
// kernel chain (seed_strand stops at K = 32 767): candidates equal the reference's also there (test_reads_beyond_the_short_seed_numbers).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "seed_defs.h"

static int bits_for(uint32_t maxv) {
    int b = 0;
    while ((1ull << b) <= maxv) ++b;
    return b < 1 ? 1 : b;
}

// ------------------------------------------------------------------------------------------------ knobs
static SeedKnobs read_knobs(const mhip_params* P) {
    auto is_zero = [](const char* name) { const char* e = getenv(name); return e && atoi(e) == 0; };
    auto number = [](const char* name, double floor) { const char* e = getenv(name); return e ? std::max(floor, atof(e)) : 0.0; };
    const int gate = 2 * P->min_kmer_match;
    const bool filters = !is_zero("MECAT_SEED_FILTER");            // debug knob: 0 disables every relevance filter
    SeedKnobs k;
    // the filter needs a gate high enough to separate signal from random hits; below that every hit is kept
    k.filter = gate >= 6 && filters;
    k.wide_filter = gate >= 4 && gate < 6 && filters;
    k.fused = k.filter && !is_zero("MECAT_SEED_FUSED");            // debug knob: 0 sends every strand through the kernel chain
    k.fused_probe = !is_zero("MECAT_SEED_FUSED_PROBE");            // debug knob: 0 runs seed_probe up front and seed_strand copies its headers from the km_* arrays
    k.cuts = !is_zero("MECAT_SEED_CUTS");                          // debug knob: 0 walks every bucket to its end
    k.predrop = !is_zero("MECAT_SEED_PREDROP");                    // debug knob: 0 lists every gated segment
    k.fused_room = number("MECAT_SEED_FUSED_ROOM", 64.0);          // test knob
    k.batch_hits = number("MECAT_SEED_BATCH_HITS", 1e6);           // tuning knob
    return k;
}

// expected bucket hits of one query k-mer
static double hits_per_lookup(const mhip_index* idx) { return (double)idx->num_kmers / (double)NKMER + 2.0; }

// ------------------------------------------------------------------------------------------------ tables
static int table(mhip_ctx* c, const char* prefix, const char* name, size_t bytes, void** out) {
    return c->scratch((std::string(prefix) + name).c_str(), bytes, out);
}

int seed_strand_tables(mhip_ctx* c, const char* prefix, int ns, SeedArrays* T) {
    if (table(c, prefix, "hits", sizeof(uint32_t) * (size_t)ns, (void**)&T->strand_hits)) return -1;
    if (table(c, prefix, "hbase", sizeof(uint64_t) * (size_t)(ns + 1), (void**)&T->hit_base)) return -1;
    if (table(c, prefix, "nseg", sizeof(uint32_t) * (size_t)ns, (void**)&T->nseg)) return -1;
    if (table(c, prefix, "nrec", sizeof(uint32_t) * (size_t)ns, (void**)&T->nrec)) return -1;
    if (table(c, prefix, "ngated", sizeof(uint32_t) * (size_t)ns, (void**)&T->ngated)) return -1;
    return 0;
}

int seed_hit_tables(mhip_ctx* c, const char* prefix, size_t cap, SeedArrays* T) {
    if (table(c, prefix, "ent", sizeof(uint32_t) * cap, (void**)&T->ent)) return -1;
    if (table(c, prefix, "entfin", sizeof(uint32_t) * cap, (void**)&T->ent_fin)) return -1;
    if (table(c, prefix, "escore", sizeof(uint16_t) * cap, (void**)&T->escore)) return -1;
    if (table(c, prefix, "segid", sizeof(uint32_t) * cap, (void**)&T->seg_id)) return -1;
    if (table(c, prefix, "segstart", sizeof(uint32_t) * cap, (void**)&T->seg_start)) return -1;
    if (table(c, prefix, "segscore", sizeof(int32_t) * cap, (void**)&T->seg_score)) return -1;
    if (table(c, prefix, "gated", sizeof(uint32_t) * cap, (void**)&T->gated)) return -1;
    return 0;
}

// ------------------------------------------------------------------------------------------------ one batch
// the description of the reads with local index in [ib, ie) of the selection
static int plan_batch(SeedBatch& b, mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, const ReadSel sel,
                      int ib, int ie, const mhip_params* P, const SeedKnobs& knobs, mhip_candidate* d_out, int32_t* d_counts) {
    b.c = c; b.idx = idx; b.ref = ref; b.reads = reads; b.sel = sel; b.P = P; b.knobs = knobs; b.d_out = d_out; b.d_counts = d_counts;
    b.ib = ib; b.nr = ie - ib; b.ns = 2 * b.nr;
    b.kmb.resize((size_t)b.ns);
    b.sumK = 0;
    for (int r = 0; r < b.nr; ++r) {
        const int K = kmers_of(reads->h_offs[(size_t)sel_rid(sel, ib + r)].size);
        b.kmb[(size_t)2 * r] = (uint32_t)b.sumK; b.sumK += (uint64_t)K;
        b.kmb[(size_t)2 * r + 1] = (uint32_t)b.sumK; b.sumK += (uint64_t)K;
    }
    if (b.sumK >= 0xFFFFFFFFull) { mhip_set_error("seed batch too large"); return -1; }
    // a diagonal grid cell (the query volume IS the reference volume): buckets cut behind each read's own copy
    b.recs = (ref == reads && knobs.cuts) ? index_ensure_cuts(c, idx) : nullptr;
    b.cut_step = b.recs ? idx->cut_step : 1;
    b.gate = 2 * P->min_kmer_match;
    b.nbits = bits_for((uint32_t)(ref->num_bases / ZV));
    b.hits_per_lookup = hits_per_lookup(idx);
    // (no subject can have a higher id than a query when the reference volume lies entirely before the query volume: nothing to drop)
    b.RR = RefReads{(const mhip_offset_t*)ref->d_offs, (const uint32_t*)ref->d_blk2read, ref->num_reads, ref->start_read_id, reads->start_read_id,
                    knobs.predrop && !(ref != reads && ref->start_read_id + ref->num_reads <= reads->start_read_id) ? 1 : 0, ref == reads ? 1 : 0};
    memset(&b.A, 0, sizeof(b.A));
    return 0;
}

// first k-mer slot of every strand, and "no strand has gone through seed_strand"
static int upload_km_bases(SeedBatch& b) {
    mhip_ctx* c = b.c;
    SeedArrays& A = b.A;
    const size_t ns = (size_t)b.ns;
    uint32_t* d_kmb;
    if (c->scratch("sd_kmbase", sizeof(uint32_t) * ns, (void**)&d_kmb)) return -1;
    if (c->scratch("sd_hitsall", sizeof(uint32_t) * ns, (void**)&A.strand_hits_all)) return -1;
    if (c->scratch("sd_fused", sizeof(int32_t) * ns, (void**)&A.fused)) return -1;
    A.km_base = d_kmb;
    // (b.kmb, the source of this copy, lives until seed_batch returns: behind the last host wait of the batch)
    HIPCHK(hipMemcpyAsync(d_kmb, b.kmb.data(), sizeof(uint32_t) * ns, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(A.fused, 0, sizeof(int32_t) * ns, c->stream));
    return 0;
}

// The bucket headers of every query k-mer (km_bstart, km_cnt) are what the kernel chain walks; seed_strand fetches the headers of its
// strands itself.  So with the strand pipeline on, seed_probe runs only when a strand has been left to the chain, then for the whole
// batch and without tallying the lookups a second time.
// Host waits: one in seed_run_strand, one in seed_run_chain, nothing more.  A batch has ns > 0 strands, so either the pipeline runs
// (its wait) or n_fallback stays ns > 0 and the chain runs (its wait): every path passes one of them before b goes away.
static int seed_batch(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, const ReadSel sel, int ib, int ie,
                      const mhip_params* P, const SeedKnobs& knobs, mhip_candidate* d_out, int32_t* d_counts) {
    SeedBatch b;
    if (plan_batch(b, c, idx, ref, reads, sel, ib, ie, P, knobs, d_out, d_counts)) return -1;
    if (upload_km_bases(b)) return -1;
    const bool probe_first = !knobs.fused || !knobs.fused_probe;
    if (probe_first && seed_run_probe(b, 1)) return -1;
    b.F = b.B = b.A;                 // (with the km_* arrays when the probe came first: seed_strand then copies its headers from them)
    unsigned int n_fallback = (unsigned int)b.ns;
    if (knobs.fused && seed_run_strand(b, &n_fallback)) return -1;
    if (n_fallback > 0) {
        if (!probe_first) {
            if (seed_run_probe(b, 0)) return -1;
            b.B.km_bstart = b.A.km_bstart;
            b.B.km_cnt = b.A.km_cnt;
        }
        if (seed_run_chain(b)) return -1;
    }
    if (seed_run_cand(b)) return -1;
    HIPCHK(hipGetLastError());
    return 0;
}

// reads per launch: bounded by an estimate of the bucket hits they produce.  The batch arrays cost ~54 bytes per KEPT
// hit (about one hit in seven survives the relevance filter); seed_cand runs one wave per read and is latency bound,
// so larger batches are what fills the chip.
static int next_batch_end(const mhip_index* idx, const mhip_volume* reads, const ReadSel sel, int rb, int re, const SeedKnobs& knobs) {
    const double hpl = hits_per_lookup(idx);
    double budget = knobs.filter ? 3.2e9 : knobs.wide_filter ? 1.6e9 : 400e6;   // ~25 GB of batch arrays either way (1.6e9: 5 ms more per config-2 pass, tail of the one-wave-per-read kernel)
    // With the relevance filter on and memory to spare the whole of a config-2 cell goes through in one launch of each kernel instead of
    // three (~60 GB of batch arrays; 57.7 against 58.8 ms per pass: two tails of the one-wave-per-read kernel and two host round trips less)
    if (knobs.filter) {
        size_t fr = 0, tot = 0;
        // in proportion to what is free right now (the batch arrays cost ~6 bytes per estimated hit; a third of the free memory at most:
        // several ranks folded onto one device, or another process on it, each see less and ask for less — ADVICE r03)
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) budget = std::max(budget, std::min(1.0e10, (double)fr / 3.0 / 6.0));
    }
    if (knobs.batch_hits > 0) budget = knobs.batch_hits;
    double acc = 0;
    int r = rb;
    while (r < re) {
        acc += 2.0 * (double)kmers_of(reads->h_offs[(size_t)sel_rid(sel, r)].size) * hpl;
        ++r;
        if (acc > budget || r - rb >= (1 << 20)) break;
    }
    return r;
}

extern "C" {

static int seed_selection(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, const ReadSel sel, int n,
                          const mhip_params* P, void* d_out, void* d_out_counts) {
    HIPCHK(hipSetDevice(c->device));
    if (n < 0 || sel.chunk < 1 || sel.cstride < 1 || sel.rid0 < 0 || (n > 0 && sel_rid(sel, n - 1) >= reads->num_reads)) {
        mhip_set_error("bad read selection begin %d chunk %d stride %d n %d", sel.rid0, sel.chunk, sel.cstride, n);
        return -1;
    }
    if (P->maxc < 1 || P->maxc > MAXC_LIMIT) { mhip_set_error("maxc %d outside 1..%d", P->maxc, MAXC_LIMIT); return -1; }
    if (ref->num_reads == 0) { mhip_set_error("empty reference volume"); return -1; }
    const SeedKnobs knobs = read_knobs(P);      // once per call, not cached: the environment may differ from call to call
    int ib = 0;
    while (ib < n) {
        int ie = next_batch_end(idx, reads, sel, ib, n, knobs);
        if (seed_batch(c, idx, ref, reads, sel, ib, ie, P, knobs, (mhip_candidate*)d_out + (size_t)ib * P->maxc, (int32_t*)d_out_counts + ib))
            return -1;
        ib = ie;
    }
    return 0;
}

int mhip_seed_reads_strided_dev(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin,
                                int rid_stride, int n, const mhip_params* P, void* d_out, void* d_out_counts) {
    if (n > 0 && (int64_t)rid_begin + (int64_t)(n - 1) * rid_stride >= reads->num_reads) {
        mhip_set_error("bad read selection begin %d stride %d n %d", rid_begin, rid_stride, n);
        return -1;
    }
    return seed_selection(c, idx, ref, reads, ReadSel{rid_begin, 1, rid_stride}, n, P, d_out, d_out_counts);
}

// local reads of a chunked shard (mecat_hip.h: mhip_shard_*): local index i -> read rid0 + (i / chunk) * chunk * nranks + i % chunk
int mhip_seed_reads_chunked_dev(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid0, int chunk,
                                int nranks, int n, const mhip_params* P, void* d_out, void* d_out_counts) {
    if (chunk < 1 || nranks < 1 || (int64_t)chunk * nranks > 0x7fffffff) { mhip_set_error("bad shard: chunk %d ranks %d", chunk, nranks); return -1; }
    return seed_selection(c, idx, ref, reads, ReadSel{rid0, chunk, chunk * nranks}, n, P, d_out, d_out_counts);
}

int mhip_seed_reads_dev(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin,
                        int rid_end, const mhip_params* P, void* d_out, void* d_out_counts) {
    if (rid_begin < 0 || rid_end > reads->num_reads || rid_begin > rid_end) { mhip_set_error("bad read range [%d,%d)", rid_begin, rid_end); return -1; }
    return mhip_seed_reads_strided_dev(c, idx, ref, reads, rid_begin, 1, rid_end - rid_begin, P, d_out, d_out_counts);
}

int mhip_seed_reads(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin,
                    int rid_end, const mhip_params* P, mhip_candidate* out, int32_t* out_counts) {
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)std::max(0, rid_end - rid_begin);
    if (n == 0) return 0;
    mhip_candidate* d_out;
    int32_t* d_cnt;
    if (c->scratch("sd_out", sizeof(mhip_candidate) * n * (size_t)P->maxc, (void**)&d_out)) return -1;
    if (c->scratch("sd_outcnt", sizeof(int32_t) * n, (void**)&d_cnt)) return -1;
    if (mhip_seed_reads_dev(c, idx, ref, reads, rid_begin, rid_end, P, d_out, d_cnt)) return -1;
    HIPCHK(hipMemcpyAsync(out_counts, d_cnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(mhip_candidate) * n * (size_t)P->maxc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
