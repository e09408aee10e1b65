// ref_seed.hip — seeding + candidate selection of mecat2ref, the reads-to-reference mapper (stage 1).
//
// Replaces, for one reference volume indexed with mhip_index_build (k = 13, buckets above 128 occurrences dropped: creat_ref_index +
// sumvalue_x, the reference's src/mecat2ref/mecat2ref_impl_large.cpp:53-62, 133-271) and a batch of query reads, the part of
// reference_mapping in front of its extend_candidate loop: :351-561 (round 1) and :619-825 (round 2).  The same family as asm_seed.hip
// with mecat2ref's own rules:
//   query k-mers at stride BC = min(20, 5 + len / 1000) (round 1) or 5 (round 2), (len - 13) / BC + 1 of them (transnum_buchang, :64-90);
//   segments of 1 000 (round 1) or 2 000 (round 2) 1-based positions with 20 stored seeds; the 21st seed and every later one goes
//   through insert_loc (:92-130): the pairwise DDF vote over the 21, then the new seed replaces the last one (all 21 agree), or the
//   entry with the fewest votes is dropped and the score taken back by one, or (the new seed has the fewest) the score just counts;
//   gate `index_score > 6` (round 1) / `> 4` (round 2), find_location of mecat2ref_aux.cpp:6-83 (the distance test against the read
//   length, `<=` in the last loop, best vote >= 5), second gate `< 6`; sweeps that start two segments to the left / one to the right and
//   read min(score, 20) entries; the list is the reference's binary insertion (:548-560), at most maxc entries.
// Arithmetic as the reference's text has it: find_location and insert_loc divide in f32 (`int / (int * float)`; find_location also
// subtracts the 1 in f32, insert_loc in f64) and compare with the f64 cutoff, the sweeps divide a 64-bit integer by `int * BC * 1.0` in
// f64 (a zero divisor gives inf or NaN and the comparison fails, there as here).  The file is built with -ffp-contract=off (Makefile).
//
// The segment array is VIRTUAL as in asm_seed.hip: a reference has a segment per 1 000 bases and a read touches a few hundred of them, so
// each wave has a directory (one 32-bit record number per segment, 0 = untouched) and a pool of 88-byte records handed out in order of
// first touch; record 0 is the untouched record (all zero, index -1) and is never written.  A read that needs more records than the
// pool holds is given up (count -1) and redone by a second launch whose pools hold a record per segment.  Every read starts from
// untouched segments (the reference resets score, score2 and index of the touched ones, :605-616; what it leaves in loczhi, seedno and
// seednum is unreachable behind score == 0), and the two strands have separate arrays there (fwd_database / rev_database), so the
// records go back to the pool between the strands as well.  Directories and pools are set up by every call (a directory is 4 bytes per
// segment and wave): nothing outlives a call.
//
// Mapping: one wave per query read, persistent, reads from an atomic cursor; everything order dependent in the reference's order with
// the wave's lanes inside each step (asm_seed.hip's scheme: a bucket 64 entries at a time, the first lane of a run of one segment is
// the hit that can be a seed, first-touch order by ballot prefix).  insert_loc and find_location vote with one list entry per lane.
// The segment array, the seeding loop, the vote and find_location's choice live in ref_seed_dev.h: ref_rescue.hip (stage 3) builds a
// strand's records again with the same code for its searches.
// Parity: tests/test_gpu_ref_seed.py against tests/golden/ref_cand.npz (recorded from the unmodified mecat2ref) and tests/ref_cand_ref.py.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "ref_seed_dev.h"

namespace {

__global__ __launch_bounds__(RF_BLOCK) void ref_seed(const uint32_t* __restrict__ starts, const int32_t* __restrict__ offsets, const uint32_t* __restrict__ qpac,
                                                    const uint32_t* __restrict__ qnpac, const mhip_offset_t* __restrict__ qoffs, int rid_begin, int n,
                                                    const int* __restrict__ rid_list, short* __restrict__ pool_all, uint32_t* __restrict__ dir_all,
                                                    int* __restrict__ hw_all, int* __restrict__ ilist_all, short* __restrict__ iscore_all, int* __restrict__ slotseg_all,
                                                    int nseg, int pcap, int Z, int round, int gate, double cutoff, int seqcount, int maxc,
                                                    unsigned int* __restrict__ cursor, mhip_ref_candidate* __restrict__ out, int32_t* __restrict__ out_counts) {
    __shared__ RefWaveLds lds[RF_WAVES];
    RefWaveLds& S = lds[threadIdx.x >> 6];
    const int lane = lane_id();
    const size_t gw = (size_t)blockIdx.x * RF_WAVES + (threadIdx.x >> 6);
    RfWave W;
    W.bind(gw, pool_all, dir_all, hw_all, ilist_all, iscore_all, slotseg_all, nseg, pcap, lane);
    auto rec = [&](int seg) { return W.rec(seg); };
    int* const ilist = W.ilist;
    volatile short* const iscore = W.iscore;

    while (true) {
        unsigned int u = 0;
        if (lane == 0) u = atomicAdd(cursor, 1u);
        u = __shfl(u, 0);
        if (u >= (unsigned)n) break;
        const int rid = rid_list ? rid_list[u] : rid_begin + (int)u;
        const size_t uo = (size_t)(rid - rid_begin);                       // the read's place in the output
        const int L = qoffs[rid].size;
        const int64_t qoff = qoffs[rid].offset;
        const int bcq = round ? 5 : min(20, 5 + L / 1000);                 // :361-362, :624
        const float bcf = (float)bcq;
        // (a read shorter than 13 has no k-mer; the reference's one look-up there reads past the string)
        const int K = L < MHIP_KMER_SIZE ? 0 : (L - MHIP_KMER_SIZE) / bcq + 1;
        int ncand = 0;
        bool ovf = false;                    // the read needs more records than the pool has: given up here, redone by the launch with full pools
        for (int strand = 0; strand < 2 && !ovf; ++strand) {
            int touched = 0;
            // ---- seeding (:417-453): ref_seed_dev.h
            ovf = !rf_seed_strand(W, S, starts, offsets, qpac, qnpac, qoff, L, K, bcq, bcf, Z, strand, cutoff, lane, touched);
            // ---- candidates (:456-561)
            for (int i = 0; i < touched && !ovf; ++i) {
                const int seg = ((volatile int*)ilist)[i];
                if (!(iscore[i] > gate)) continue;
                vshort* g = rec(seg);
                const int score = g[R_SCORE];
                if (score == 0) continue;
                const int prev = seg > 0 ? (int)rec(seg - 1)[R_SCORE] : 0;
                const int64_t start_loc = (int64_t)(prev > 0 ? seg - 1 : seg) * Z;
                const int np = prev > 0 ? min(prev, RF_SM) : 0, ns = min(score, RF_SM), nl = np + ns;
                if (lane < nl) {
                    if (lane < np) { S.tl[lane] = rec(seg - 1)[R_LOC + lane]; S.ts[lane] = rec(seg - 1)[R_SEED + lane]; }
                    else { S.tl[lane] = g[R_LOC + lane - np] + (prev > 0 ? Z : 0); S.ts[lane] = g[R_SEED + lane - np]; }
                }
                S.tsc[lane] = 0;
                __builtin_amdgcn_wave_barrier();
                rf_vote<false>(S, nl, lane, bcf, cutoff, L);
                int rep_loc, loc0, loc1;
                const bool flag = rf_select(S, nl, L, bcf, cutoff, loc0, loc1, rep_loc);
                if (!flag) continue;
                const int vote = S.tsc[rep_loc];
                if (vote < 6) continue;                                  // :496
                const int loc_seed = S.ts[rep_loc];
                mhip_ref_candidate c;
                const int64_t loc_list = start_loc + loc0;
                c.loc1 = loc_list;
                c.loc2 = (int64_t)(loc1 - 1) * bcq;
                c.left1 = c.loc1 + MHIP_KMER_SIZE - 1; c.right1 = (int64_t)seqcount - c.loc1;
                c.left2 = c.loc2 + MHIP_KMER_SIZE - 1; c.right2 = (int64_t)L - c.loc2;
                c.num1 = (int)(c.left1 >= c.left2 ? c.left2 : c.left1);
                c.num2 = (int)(c.right1 >= c.right2 ? c.right2 : c.right1);
                int seedcount = 0;
                // sweeps (:521-543): min(score, 20) entries of every touched segment in reach; a segment with more than 0.4 of them on the
                // candidate's diagonal is taken out (score = 0), which later steps of the same loops and later candidates see
                for (int useg = seg - 2, kk = c.num1 / Z; useg >= 0 && kk >= 0; --useg, --kk) {
                    vshort* o = rec(useg);
                    const int osc = o[R_SCORE];
                    if (osc <= 0) continue;
                    const int scnt = min(osc, RF_SM);
                    const int64_t sl = (int64_t)useg * Z;
                    bool q = false;
                    if (lane < scnt) q = fabs((double)(loc_list - sl - (int64_t)o[R_LOC + lane]) / ((double)((loc_seed - (int)o[R_SEED + lane]) * bcq) * 1.0) - 1.0) < cutoff;
                    const int agree = (int)__popcll(__ballot(q));
                    seedcount += agree;
                    if (agree * 1.0 / scnt > 0.4 && lane == 0) o[R_SCORE] = 0;
                }
                for (int useg = seg + 1, kk = c.num2 / Z; kk > 0 && useg < nseg + 8; ++useg, --kk) {
                    vshort* o = rec(useg);
                    const int osc = o[R_SCORE];
                    if (osc <= 0) continue;
                    const int scnt = min(osc, RF_SM);
                    const int64_t sl = (int64_t)useg * Z;
                    bool q = false;
                    if (lane < scnt) q = fabs((double)(sl + (int64_t)o[R_LOC + lane] - loc_list) / ((double)(((int)o[R_SEED + lane] - loc_seed) * bcq) * 1.0) - 1.0) < cutoff;
                    const int agree = (int)__popcll(__ballot(q));
                    seedcount += agree;
                    if (agree * 1.0 / scnt > 0.4 && lane == 0) o[R_SCORE] = 0;
                }
                rf_sync();
                c.score = vote + seedcount;
                c.chain = strand;
                // stable insertion into the descending list of at most maxc entries (:548-560)
                int lo = 0, hi = ncand - 1;
                while (lo <= hi) {
                    const int mid = (lo + hi) / 2;
                    if (mid >= ncand || S.cand[mid].score < c.score) hi = mid - 1; else lo = mid + 1;
                }
                const int top = ncand < maxc ? ncand - 1 : ncand - 2;        // last entry that moves one place down
                __builtin_amdgcn_wave_barrier();
                // (entries hi + 1 .. top move to hi + 2 .. top + 1: every lane reads its entries first, then writes)
                mhip_ref_candidate mv[2];
                bool has[2];
                for (int q = 0; q < 2; ++q) {
                    const int j = hi + 1 + lane + 64 * q;
                    has[q] = j <= top;
                    if (has[q]) mv[q] = S.cand[j];
                }
                __builtin_amdgcn_wave_barrier();
                for (int q = 0; q < 2; ++q) {
                    const int j = hi + 1 + lane + 64 * q;
                    if (has[q]) S.cand[j + 1] = mv[q];
                }
                if (lane == 0 && hi + 1 < maxc) S.cand[hi + 1] = c;
                if (ncand < maxc) ++ncand;
                __builtin_amdgcn_wave_barrier();
            }
            // ---- the strand is done (or given up): its records go back to the pool
            W.release(lane);
        }
        if (ovf) ncand = 0;
        for (int j = lane; j < ncand; j += 64) out[uo * (size_t)maxc + j] = S.cand[j];
        if (lane == 0) {
            out_counts[uo] = ovf ? -1 : ncand;
            atomicMax(cursor + 4, (unsigned int)W.hw);
            if (ovf) atomicAdd(cursor + 5, 1u);
        }
        rf_sync();
    }
    if (lane == 0) hw_all[gw] = W.hw;
}

int64_t g_last_stats[4] = {0, 0, 0, 0};

// the stage for reads [rid_begin, rid_end): results in the DEVICE buffers d_out [n][maxc], d_cnt [n]
int ref_seed_run(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                 const mhip_ref_seed_params* p, mhip_ref_candidate* d_out, int32_t* d_cnt) {
    HIPCHK(hipSetDevice(c->device));
    if (p->maxc < 1 || p->maxc > RF_MAXC) { mhip_set_error("mhip_ref_seed_reads: list length %d outside 1..%d", p->maxc, RF_MAXC); return -1; }
    if (p->round != 0 && p->round != 1) { mhip_set_error("mhip_ref_seed_reads: round %d (0: first, 1: second)", p->round); return -1; }
    if (rid_begin < 0 || rid_end > reads->num_reads || rid_begin > rid_end) { mhip_set_error("bad read range [%d,%d)", rid_begin, rid_end); return -1; }
    if (idx->max_bucket != MAX_BUCKET) { mhip_set_error("mhip_ref_seed_reads needs an index built with mhip_index_build (bucket cap 128), not %d", idx->max_bucket); return -1; }
    if (idx->num_bases != ref->num_bases) { mhip_set_error("the index was not built from this reference volume"); return -1; }
    for (int r = rid_begin; r < rid_end; ++r)
        if (reads->h_offs[r].size >= RF_RM) {
            mhip_set_error("mhip_ref_seed_reads: read %d has %d letters; mecat2ref's read buffers hold fewer than %d", r, reads->h_offs[r].size, RF_RM);
            return -1;
        }
    const int n = rid_end - rid_begin;
    g_last_stats[0] = n; g_last_stats[1] = g_last_stats[2] = g_last_stats[3] = 0;
    if (n == 0) return 0;
    const int Z = p->round ? 2000 : 1000, gate = p->round ? 4 : 6;
    const int nseg = ref->num_bases / Z + 5;
    RfPools P;
    if (rf_pools_first(c, nseg, n, &P)) return -1;
    const size_t waves = P.waves;
    const int pcap = P.pcap;
    unsigned int* d_cur = P.cur;
    LAUNCH(c, "ref_seed", ref_seed, P.grid, RF_BLOCK, 0, (const uint32_t*)idx->d_starts, (const int32_t*)idx->d_offsets, (const uint32_t*)reads->d_pac,
           (const uint32_t*)reads->d_npac, (const mhip_offset_t*)reads->d_offs, rid_begin, n, (const int*)nullptr, P.pool, P.dir, P.hw, P.ilist, P.iscore, P.slotseg,
           nseg, pcap, Z, p->round, gate, p->ddfs_cutoff, ref->num_bases, p->maxc, d_cur, d_out, d_cnt);
    HIPCHK(hipGetLastError());
    unsigned int st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(st, d_cur, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    g_last_stats[1] = st[5]; g_last_stats[2] = (int64_t)waves; g_last_stats[3] = pcap;
    if (getenv("MECAT_REF_STATS")) fprintf(stderr, "[ref_seed] %d reads on %zu waves, pools of %d records: most records a wave initialised %u, reads given up %u\n", n, waves, pcap, st[4], st[5]);
    if (st[5]) {
        // the reads that ran out of records, again, with pools that cannot (one record per segment): few waves, their own pool buffers;
        // directories (all zero again) and output are the first launch's
        std::vector<int32_t> cnt((size_t)n);
        HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        std::vector<int> redo;
        for (int i = 0; i < n; ++i)
            if (cnt[i] < 0) redo.push_back(rid_begin + i);
        RfPools F;
        int* d_redo;
        if (rf_pools_full(c, P, redo.size(), "ref_seed", &F)) return -1;
        if (c->scratch("rf_redo", sizeof(int) * redo.size(), (void**)&d_redo)) return -1;
        HIPCHK(hipMemcpyAsync(d_redo, redo.data(), sizeof(int) * redo.size(), hipMemcpyHostToDevice, c->stream));
        LAUNCH(c, "ref_seed_full", ref_seed, F.grid, RF_BLOCK, 0, (const uint32_t*)idx->d_starts, (const int32_t*)idx->d_offsets, (const uint32_t*)reads->d_pac,
               (const uint32_t*)reads->d_npac, (const mhip_offset_t*)reads->d_offs, rid_begin, (int)redo.size(), (const int*)d_redo, F.pool, F.dir, F.hw, F.ilist,
               F.iscore, F.slotseg, nseg, F.pcap, Z, p->round, gate, p->ddfs_cutoff, ref->num_bases, p->maxc, d_cur, d_out, d_cnt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));          // (`redo` is read by the copy above until here)
    }
    return 0;
}

}  // namespace

extern "C" {

void mhip_ref_seed_params_default(mhip_ref_seed_params* p, int tech) {
    (void)tech;
    p->maxc = 10;          // kDefaultNumCandidates, mecat2ref.cpp:18
    p->round = 0;
    // mecat2ref_impl_large.cpp:13-15 names 0.25 for PacBio and 0.1 for nanopore and never assigns the second: `ddfs_cutoff` stays 0.25
    // whatever -x says (the recorded nanopore lists equal the PacBio ones), so that is the default of both technologies here
    p->ddfs_cutoff = 0.25;
}

int mhip_ref_seed_reads_dev(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                            const mhip_ref_seed_params* p, mhip_ref_candidate* d_out, int32_t* d_out_counts) {
    return ref_seed_run(c, idx, ref, reads, rid_begin, rid_end, p, d_out, d_out_counts);
}

int mhip_ref_seed_reads(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                        const mhip_ref_seed_params* p, mhip_ref_candidate* out, int32_t* out_counts) {
    HIPCHK(hipSetDevice(c->device));
    const int n = rid_end - rid_begin;
    if (n <= 0 || p->maxc < 1) return ref_seed_run(c, idx, ref, reads, rid_begin, rid_end, p, nullptr, nullptr);
    mhip_ref_candidate* d_out;
    int32_t* d_cnt;
    if (c->scratch("rf_out", sizeof(mhip_ref_candidate) * (size_t)n * (size_t)p->maxc, (void**)&d_out)) return -1;
    if (c->scratch("rf_cnt", sizeof(int32_t) * (size_t)n, (void**)&d_cnt)) return -1;
    if (ref_seed_run(c, idx, ref, reads, rid_begin, rid_end, p, d_out, d_cnt)) return -1;
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(mhip_ref_candidate) * (size_t)n * (size_t)p->maxc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_counts, d_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

void mhip_ref_seed_stats(int64_t out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = g_last_stats[i];
}

}  // extern "C"
