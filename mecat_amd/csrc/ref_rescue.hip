// ref_rescue.hip — mecat2ref's clipped-alignment rescue and its result order on the device (stage 3).  Both technologies:
// only the extension behind the rescue candidates differs (mhip_ref_rescue_run: DiffAligner, mhip_ref_xrescue_run: XdropAligner).
//
// Replaces what reference_mapping does with a read's results between its extension loop and the result file
// (mecat2ref/mecat2ref_impl_large.cpp:584-603 for round 1, :847-866 for round 2):
//   rescue_clipped_align  mecat2ref/mecat2ref_aux.cpp:308-452 with is_full_align / AlignInfoContained (mecat2ref_aux.h:22-42),
//                         find_left_clipped_candidate / find_right_clipped_candidate / fill_clipped_candidate (:185-274) and
//                         is_left_clipped_align / is_right_clipped_align (:276-306)
//   output_results        :454-473
// Kernels, in call order:
//   ref_rescue_prep    one lane per read: the sort by aligned read length (std::sort on at most 16 elements is libstdc++'s insertion
//                      sort: stable), the containment filter with its compaction and the full-alignment test of the longest entry
//                      (:328-341): the state the searches start from, and the list of the reads that go on;
//   ref_rescue_find    one wave per read that goes on: the strands' segment records again (ref_seed_dev.h) and the searches (below);
//   (ref_extend.hip)   the rescue candidates, at most 6 per read, through the extension into the second buffer set;
//   ref_rescue_finish  one lane per read: the attach tests on the rescue results in call order (:380-399, :416-435), the second sort
//                      with the full-alignment cut (:438-451) and output_results' walk: the slots of the records in printed order.
// The chaining loop at :343-357 asks for `prev_id != -1` / `next_id != -1` on entries that all hold -1 there, so it never does
// anything; it is not built.  Ids are the tool's: entry t of the read's ok results in list order has id t, an ok rescue result takes
// the next id whether it is attached or not.  A record is named by its slot: [0, maxc) = slot of the first list, maxc + j = rescue
// slot j.  Lists longer than 10 are refused: beyond 16 elements the order of equal lengths is libstdc++'s introsort's.
// Parity: tests/test_gpu_ref_rescue.py against tests/golden/ref_rescue.npz (recorded from the unmodified functions on hand-made arrays
// and segment records), tests/test_gpu_ref_rescue_chain.py (seed -> extend -> rescue) against tests/ref_rescue_ref.py.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include <vector>

#include "ref_extend.h"
#include "ref_seed_dev.h"

#define RR_MAXC 10                   // longest first list (the tool's default -n)
#define RR_TRIES 6                   // rescue candidates of a read: left and right of its first three entries
#define RR_ENT (RR_MAXC + RR_TRIES)  // AlignInfo alns[MAXC + 6], mecat2ref_impl_large.cpp:311
#define RR_BLOCK 64

namespace {

struct RrEntry { int qoff, qend, qdir, id, prev, next, parent, slot; int64_t soff, send; };   // prev / next: slots, not ids

__device__ __forceinline__ RrEntry rr_entry(const mhip_ref_result& r, int id, int slot) {
    RrEntry e;
    e.qoff = r.qb; e.qend = r.qe; e.qdir = r.chain; e.soff = r.sb; e.send = r.se;
    e.id = id; e.slot = slot; e.prev = e.next = e.parent = -1;
    return e;
}

// is_full_align (mecat2ref_aux.h:22-26): int against int * 0.9 in f64
__device__ __forceinline__ bool rr_full(int qoff, int qend, int qs) { return (double)(qend - qoff) >= (double)qs * 0.9; }

// AlignInfoContained(a, b) (mecat2ref_aux.h:28-42)
__device__ __forceinline__ bool rr_contained(const RrEntry& a, const RrEntry& b) {
    const int extra = 100;
    return a.qdir == b.qdir && b.qoff + extra >= a.qoff && b.qend <= a.qend + extra && b.soff + extra >= a.soff && b.send <= a.send + extra;
}

__device__ __forceinline__ int64_t rr_abs(int64_t v) { return v < 0 ? -v : v; }

// is_left_clipped_align(a, b) (mecat2ref_aux.cpp:276-290); abs() of the read-side difference is int, of the reference side long
__device__ __forceinline__ bool rr_left(const RrEntry& a, const RrEntry& b) {
    if (a.qdir != b.qdir) return false;
    if (abs(b.qend - a.qoff) <= 200 && a.soff - b.send > -200 && a.soff - b.send < 10000) return true;
    if (rr_abs(b.send - a.soff) <= 200 && a.qoff - b.qend > -200 && a.qoff - b.qend < 10000) return true;
    return false;
}

// is_right_clipped_align(a, b) (:292-306)
__device__ __forceinline__ bool rr_right(const RrEntry& a, const RrEntry& b) {
    if (a.qdir != b.qdir) return false;
    if (abs(a.qend - b.qoff) <= 200 && b.soff - a.send > -200 && b.soff - a.send < 10000) return true;
    if (rr_abs(a.send - b.soff) <= 200 && b.qoff - a.qend > -200 && b.qoff - a.qend < 10000) return true;
    return false;
}

// std::sort(alnv, alnv + n) with operator< = longer aligned read stretch first, n <= 16: insertion, equal lengths keep their order
__device__ __forceinline__ void rr_sort(RrEntry* e, int n) {
    for (int i = 1; i < n; ++i) {
        const RrEntry v = e[i];
        int j = i;
        while (j > 0 && v.qend - v.qoff > e[j - 1].qend - e[j - 1].qoff) { e[j] = e[j - 1]; --j; }
        e[j] = v;
    }
}

__global__ __launch_bounds__(RR_BLOCK) void ref_rescue_prep(const mhip_ref_result* __restrict__ res, int n, int maxc, mhip_ref_rescue_state* __restrict__ state,
                                                            int* __restrict__ go_list, unsigned int* __restrict__ go_count) {
    const int r = blockIdx.x * RR_BLOCK + threadIdx.x;
    if (r >= n) return;
    RrEntry e[RR_MAXC];
    int naln = 0, qs = 0;
    for (int s = 0; s < maxc; ++s) {
        const mhip_ref_result x = res[(size_t)r * maxc + s];
        if (!x.ok) continue;
        qs = x.qs;
        e[naln] = rr_entry(x, naln, s);
        ++naln;
    }
    const int nres = naln;
    rr_sort(e, naln);
    bool valid[RR_MAXC];
    for (int i = 0; i < RR_MAXC; ++i) valid[i] = true;
    for (int i = 0; i + 1 < naln; ++i) {
        if (!valid[i]) continue;
        for (int j = i + 1; j < naln; ++j)
            if (valid[j] && rr_contained(e[i], e[j])) valid[j] = false;
    }
    mhip_ref_rescue_state st;
    for (int i = 0; i < 16; ++i) st.slot[i] = st.id[i] = -1;
    int k = 0;
    bool full0 = false;
    for (int i = 0; i < naln; ++i) {
        if (!valid[i]) continue;
        if (k == 0) full0 = rr_full(e[i].qoff, e[i].qend, qs);
        st.slot[k] = (int8_t)e[i].slot;
        st.id[k] = (int8_t)e[i].id;
        ++k;
    }
    st.naln = k;
    st.nres = nres;
    st.qs = qs;
    st.go_on = k > 0 && !full0;           // (with no entry the tool tests an entry it never wrote; its loops then run zero times either way)
    state[r] = st;
    if (go_list && st.go_on) go_list[atomicAdd(go_count, 1u)] = r;          // (the order does not matter: every read writes its own slots)
}

// meta[j] of rescue slot j: owner entry (its place in the state's order, 0..2) | side << 8 (0 left, 1 right)
__global__ __launch_bounds__(RR_BLOCK) void ref_rescue_finish(const mhip_ref_result* __restrict__ res, const mhip_ref_rescue_state* __restrict__ state,
                                                              const int32_t* __restrict__ rcount, const int32_t* __restrict__ meta,
                                                              const mhip_ref_result* __restrict__ rres, int n, int maxc, int num_output,
                                                              int32_t* __restrict__ out_slots, int32_t* __restrict__ out_counts) {
    const int r = blockIdx.x * RR_BLOCK + threadIdx.x;
    if (r >= n) return;
    const mhip_ref_rescue_state st = state[r];
    RrEntry e[RR_ENT];
    int naln = min(max(st.naln, 0), RR_MAXC);
    for (int i = 0; i < naln; ++i) {
        const int s = min(max((int)st.slot[i], 0), maxc - 1);
        e[i] = rr_entry(res[(size_t)r * maxc + s], st.id[i], s);
    }
    if (st.go_on) {
        int k = 0, nid = st.nres;
        const int nr = min(max(rcount[r], 0), RR_TRIES);
        for (int j = 0; j < nr; ++j) {
            const mhip_ref_result x = rres[(size_t)r * RR_TRIES + j];
            if (!x.ok) continue;
            const int m = meta[(size_t)r * RR_TRIES + j], owner = m & 0xff, side = (m >> 8) & 1;
            if (owner >= naln || owner >= 3) continue;
            // the new entry is written behind the attached ones; one that is not attached is overwritten by the next, its id stays used
            RrEntry ai = rr_entry(x, nid++, maxc + j);
            if (!side ? rr_left(e[owner], ai) : rr_right(e[owner], ai)) {
                ai.parent = e[owner].id;
                if (!side) e[owner].prev = ai.slot; else e[owner].next = ai.slot;
                e[naln + k] = ai;           // (naln <= 10, k <= 5 here)
                ++k;
            }
        }
        if (k) {
            naln += k;
            rr_sort(e, naln);
            int nfull = 0;
            for (int i = 0; i < naln; ++i)
                if (rr_full(e[i].qoff, e[i].qend, st.qs)) { e[i].parent = e[i].prev = e[i].next = -1; ++nfull; }
            if (nfull) naln = nfull;          // (the full ones are the longest: the head of the sorted array)
        }
    }
    // output_results
    int32_t* o = out_slots + (size_t)r * 3 * num_output;
    int w = 0, groups = 0;
    for (int i = 0; i < naln && groups < num_output; ++i) {
        if (e[i].parent != -1) continue;
        o[w++] = e[i].slot;
        if (e[i].prev != -1) o[w++] = e[i].prev;
        if (e[i].next != -1) o[w++] = e[i].next;
        ++groups;
    }
    out_counts[r] = w;
    for (; w < 3 * num_output; ++w) o[w] = -1;
}

// tech: the technology of the entry point (0: the PacBio calls, 1: mhip_ref_xrescue_run*); params.tech must name the same one
int rr_check(const char* who, const mhip_ref_rescue_params* p, int n, int tech = 0) {
    if (p->tech != tech) {
        mhip_set_error("%s: technology %d: this call is %s mode (%d); %s", who, p->tech, tech ? "nanopore" : "PacBio", tech,
                       tech ? "PacBio mode is mhip_ref_rescue_run" : "nanopore mode is mhip_ref_xrescue_run");
        return -1;
    }
    if (p->maxc < 1 || p->maxc > RR_MAXC) { mhip_set_error("%s: list length %d outside 1..%d (the order of equal lengths beyond 16 entries is not reproduced)", who, p->maxc, RR_MAXC); return -1; }
    if (p->num_output < 1) { mhip_set_error("%s: num_output %d below 1", who, p->num_output); return -1; }
    if (p->round != 0 && p->round != 1) { mhip_set_error("%s: round %d (0: first, 1: second)", who, p->round); return -1; }
    if (n < 0) { mhip_set_error("%s: %d reads", who, n); return -1; }
    return 0;
}

// ---------------------------------------------------------------- the searches
// One wave per read that goes on.  For each strand that owns one of the read's first three entries the strand's segment records are built
// again by the seeding loop ref_seed runs (ref_seed_dev.h) — `score2` of the tool is the record's score as that loop leaves it, loczhi /
// seedno are not touched afterwards — then find_left_clipped_candidate / find_right_clipped_candidate (:214-274) scan their segments with
// the wave's lanes and fill_clipped_candidate (:185-212) votes over the best one.  The searches read nothing the attach step writes (an
// entry's prev_id / next_id are set by its own side's try alone), so all of a read's candidates are found before any is extended; they
// are packed in the tool's call order (entry 0 left, entry 0 right, entry 1 left, ...), meta = owner entry | side << 8.
// A read that needs more records than the pool has gets count -1 and is redone by a launch with full pools (rid_list), as in ref_seed.
__device__ __forceinline__ int rr_wave_max(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(RF_BLOCK) void ref_rescue_find(const uint32_t* __restrict__ starts, const int32_t* __restrict__ offsets, const uint32_t* __restrict__ qpac,
                                                           const uint32_t* __restrict__ qnpac, const mhip_offset_t* __restrict__ qoffs, int rid_begin, int nlist,
                                                           const int* __restrict__ list, short* __restrict__ pool_all, uint32_t* __restrict__ dir_all,
                                                           int* __restrict__ hw_all, int* __restrict__ ilist_all, short* __restrict__ iscore_all,
                                                           int* __restrict__ slotseg_all, int nseg, int pcap, int Z, int round, double cutoff, int64_t ref_size,
                                                           int maxc, unsigned int* __restrict__ cursor, const mhip_ref_result* __restrict__ res,
                                                           const mhip_ref_rescue_state* __restrict__ state, mhip_ref_candidate* __restrict__ out,
                                                           int32_t* __restrict__ out_counts, int32_t* __restrict__ out_meta) {
    typedef RefWaveLdsT<RR_TRIES> Lds;                                     // the vote's lists and the read's six candidate slots
    __shared__ Lds lds[RF_WAVES];
    Lds& S = lds[threadIdx.x >> 6];
    const int lane = lane_id();
    const size_t gw = (size_t)blockIdx.x * RF_WAVES + (threadIdx.x >> 6);
    RfWave W;
    W.bind(gw, pool_all, dir_all, hw_all, ilist_all, iscore_all, slotseg_all, nseg, pcap, lane);
    while (true) {
        unsigned int u = 0;
        if (lane == 0) u = atomicAdd(cursor, 1u);
        u = __shfl(u, 0);
        if (u >= (unsigned)nlist) break;
        const int uo = list[u];                                            // the read's place in the batch
        const int rid = rid_begin + uo;
        const mhip_ref_rescue_state st = state[uo];
        const int L = qoffs[rid].size;
        const int64_t qoff = qoffs[rid].offset;
        const int bcq = round ? 5 : min(20, 5 + L / 1000);
        const float bcf = (float)bcq;
        const int K = L < MHIP_KMER_SIZE ? 0 : (L - MHIP_KMER_SIZE) / bcq + 1;
        const int nent = min(max(st.naln, 0), 3);
        mhip_ref_result ent[3];
        for (int e = 0; e < 3; ++e)
            if (e < nent) ent[e] = res[(size_t)uo * maxc + min(max((int)st.slot[e], 0), maxc - 1)];
        unsigned found = 0;                                                // bit 2 * entry + side; the candidates wait in S.cand[]
        bool ovf = false;
        for (int strand = 0; strand < 2 && !ovf; ++strand) {
            bool owns = false;
            for (int e = 0; e < 3; ++e) owns |= e < nent && ent[e].chain == strand;
            if (!owns) continue;
            int touched = 0;
            ovf = !rf_seed_strand(W, S, starts, offsets, qpac, qnpac, qoff, L, K, bcq, bcf, Z, strand, cutoff, lane, touched);
            for (int t = 0; t < 6 && !ovf; ++t) {
                const int e = t >> 1, side = t & 1;
                if (e >= nent || ent[e].chain != strand) continue;
                const mhip_ref_result a = ent[e];
                // the segments to scan: `first`, then `step` further per look, `steps` of them
                int first, step, steps;
                if (!side) {
                    if (a.qb <= 2000 || a.sb <= 2000) continue;           // CLIPPED
                    const int n2 = (int)(a.sb / Z);
                    first = n2 - 1; step = -1;
                    steps = min(min(a.qb / Z, n2) + 1, first + 1);         // `n >= 0 && n2 >= 0`
                } else {
                    if (L - a.qe <= 2000 || ref_size - a.se <= 2000) continue;
                    first = (int)(a.se / Z) + 1; step = 1;
                    steps = min(min((L - a.qe) / Z, (int)((ref_size - a.se) / Z)) + 1, nseg + 8 - first);
                }
                int best = 0, bseg = -1;                                   // the largest score2, the first one met (`>`)
                for (int i0 = 0; i0 < steps; i0 += 64) {
                    const int i = i0 + lane;
                    const int sc = i < steps ? (int)W.rec(first + step * i)[R_SCORE] : 0;
                    const int m = rr_wave_max(sc);
                    if (m > best) {
                        best = m;
                        bseg = first + step * (i0 + __ffsll((long long)__ballot(sc == m)) - 1);
                    }
                }
                if (bseg < 0 || !(best > 4)) continue;
                vshort* g = W.rec(bseg);
                const int nl = min(best, RF_SM);
                if (lane < nl) { S.tl[lane] = g[R_LOC + lane]; S.ts[lane] = g[R_SEED + lane]; }
                S.tsc[lane] = 0;
                __builtin_amdgcn_wave_barrier();
                rf_vote<false>(S, nl, lane, bcf, cutoff, L);
                int rep_loc, loc0, loc1;
                if (!rf_select(S, nl, L, bcf, cutoff, loc0, loc1, rep_loc)) continue;
                if (lane == 0) {
                    mhip_ref_candidate c;
                    c.score = S.tsc[rep_loc];
                    c.chain = a.chain;
                    c.loc1 = (int64_t)bseg * Z + loc0;
                    c.loc2 = (int64_t)(loc1 - 1) * bcq;
                    // (fill_clipped_candidate leaves the other members unset; they are filled as the candidate stage fills them)
                    c.left1 = c.loc1 + MHIP_KMER_SIZE - 1; c.right1 = ref_size - c.loc1;
                    c.left2 = c.loc2 + MHIP_KMER_SIZE - 1; c.right2 = (int64_t)L - c.loc2;
                    c.num1 = (int)(c.left1 >= c.left2 ? c.left2 : c.left1);
                    c.num2 = (int)(c.right1 >= c.right2 ? c.right2 : c.right1);
                    S.cand[t] = c;
                }
                found |= 1u << t;
                __builtin_amdgcn_wave_barrier();
            }
            W.release(lane);
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < 6 && !ovf && (found >> lane & 1u)) {
            const int j = __popc(found & ((1u << lane) - 1u));
            out[(size_t)uo * RR_TRIES + j] = S.cand[lane];
            out_meta[(size_t)uo * RR_TRIES + j] = (lane >> 1) | (lane & 1) << 8;
        }
        if (lane == 0) {
            out_counts[uo] = ovf ? -1 : __popc(found);
            atomicMax(cursor + 4, (unsigned int)W.hw);
            if (ovf) atomicAdd(cursor + 5, 1u);
        }
        rf_sync();
    }
    if (lane == 0) hw_all[gw] = W.hw;
}

int64_t g_rescue_stats[4] = {0, 0, 0, 0};

// the stage for reads [rid_begin, rid_end) on DEVICE results d_res [n][maxc]
int rescue_run(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, const mhip_ref_rescue_params* p,
               const mhip_ref_result* d_res, int64_t* total_words, int aligner) {
    const int n = rid_end - rid_begin;
    c->rr_n = 0;
    g_rescue_stats[0] = n; g_rescue_stats[1] = g_rescue_stats[2] = g_rescue_stats[3] = 0;
    if (total_words) *total_words = 0;
    if (n == 0) return 0;
    const int Z = p->round ? 2000 : 1000;
    const int nseg = ref->num_bases / Z + 5;
    mhip_ref_rescue_state* d_st;
    int32_t *d_list, *d_rcount, *d_meta, *d_os, *d_oc;
    mhip_ref_candidate* d_cands;
    const size_t no = (size_t)n * 3 * p->num_output;
    if (c->scratch("rr_state", sizeof(mhip_ref_rescue_state) * (size_t)n, (void**)&d_st)) return -1;
    if (c->scratch("rr_list", sizeof(int32_t) * (size_t)n, (void**)&d_list)) return -1;
    if (c->scratch("rr_cands", sizeof(mhip_ref_candidate) * (size_t)n * RR_TRIES, (void**)&d_cands)) return -1;
    if (c->scratch("rr_rcount", sizeof(int32_t) * (size_t)n, (void**)&d_rcount)) return -1;
    if (c->scratch("rr_meta", sizeof(int32_t) * (size_t)n * RR_TRIES, (void**)&d_meta)) return -1;
    if (c->scratch("rr_out_slots", sizeof(int32_t) * no, (void**)&d_os)) return -1;
    if (c->scratch("rr_out_counts", sizeof(int32_t) * (size_t)n, (void**)&d_oc)) return -1;
    RfPools P;
    if (rf_pools_first(c, nseg, n, &P)) return -1;
    HIPCHK(hipMemsetAsync(d_rcount, 0, sizeof(int32_t) * (size_t)n, c->stream));
    LAUNCH(c, "ref_rescue_prep", ref_rescue_prep, (n + RR_BLOCK - 1) / RR_BLOCK, RR_BLOCK, 0, d_res, n, p->maxc, d_st, d_list, P.cur + 8);
    HIPCHK(hipGetLastError());
    unsigned int st[16];
    HIPCHK(hipMemcpyAsync(st, P.cur, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int nlist = (int)st[8];
    g_rescue_stats[1] = nlist;
    std::vector<int32_t> cnt((size_t)n, 0);
    if (nlist > 0) {
        const unsigned grid = std::min<unsigned>(P.grid, (unsigned)((nlist + RF_WAVES - 1) / RF_WAVES));
        LAUNCH(c, "ref_rescue_find", ref_rescue_find, grid, RF_BLOCK, 0, (const uint32_t*)idx->d_starts, (const int32_t*)idx->d_offsets, (const uint32_t*)reads->d_pac,
               (const uint32_t*)reads->d_npac, (const mhip_offset_t*)reads->d_offs, rid_begin, nlist, (const int*)d_list, P.pool, P.dir, P.hw, P.ilist, P.iscore,
               P.slotseg, nseg, P.pcap, Z, p->round, p->ddfs_cutoff, (int64_t)ref->num_bases, p->maxc, P.cur, d_res, (const mhip_ref_rescue_state*)d_st, d_cands,
               d_rcount, d_meta);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(st, P.cur, sizeof(st), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(cnt.data(), d_rcount, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (st[5]) {
            std::vector<int> redo;
            for (int i = 0; i < n; ++i)
                if (cnt[(size_t)i] < 0) redo.push_back(i);
            g_rescue_stats[3] = (int64_t)redo.size();
            RfPools F;
            int* d_redo;
            if (rf_pools_full(c, P, redo.size(), "ref_rescue_find", &F)) return -1;
            if (c->scratch("rf_redo", sizeof(int) * redo.size(), (void**)&d_redo)) return -1;
            HIPCHK(hipMemcpyAsync(d_redo, redo.data(), sizeof(int) * redo.size(), hipMemcpyHostToDevice, c->stream));
            LAUNCH(c, "ref_rescue_find_full", ref_rescue_find, F.grid, RF_BLOCK, 0, (const uint32_t*)idx->d_starts, (const int32_t*)idx->d_offsets,
                   (const uint32_t*)reads->d_pac, (const uint32_t*)reads->d_npac, (const mhip_offset_t*)reads->d_offs, rid_begin, (int)redo.size(), (const int*)d_redo,
                   F.pool, F.dir, F.hw, F.ilist, F.iscore, F.slotseg, nseg, F.pcap, Z, p->round, p->ddfs_cutoff, (int64_t)ref->num_bases, p->maxc, F.cur, d_res,
                   (const mhip_ref_rescue_state*)d_st, d_cands, d_rcount, d_meta);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(cnt.data(), d_rcount, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));          // (`redo` is read by the copy above until here)
        }
    }
    for (int i = 0; i < n; ++i) {
        if (cnt[(size_t)i] < 0) { mhip_set_error("ref_rescue_find: read %d ran out of segment records with a record per segment", rid_begin + i); return -1; }
        g_rescue_stats[2] += cnt[(size_t)i];
    }
    // the rescue candidates through the extension, into the second buffer set: the first extension's results stay where they are
    if (ref_extend_run(c, ref, reads, rid_begin, rid_end, RR_TRIES, aligner, d_cands, d_rcount, total_words, 1)) return -1;
    mhip_ref_result* d_rres;
    if (scratch_set(c, "rx_res", 1, 0, (void**)&d_rres)) return -1;
    LAUNCH(c, "ref_rescue_finish", ref_rescue_finish, (n + RR_BLOCK - 1) / RR_BLOCK, RR_BLOCK, 0, d_res, (const mhip_ref_rescue_state*)d_st, (const int32_t*)d_rcount,
           (const int32_t*)d_meta, (const mhip_ref_result*)d_rres, n, p->maxc, p->num_output, d_os, d_oc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    c->rr_n = n; c->rr_num_output = p->num_output;
    return 0;
}

int rr_check_run(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, const mhip_ref_rescue_params* p,
                 int tech = 0) {
    if (rid_begin < 0 || rid_end > reads->num_reads || rid_begin > rid_end) { mhip_set_error("mhip_ref_rescue_run: bad read range [%d,%d)", rid_begin, rid_end); return -1; }
    if (rr_check(tech ? "mhip_ref_xrescue_run" : "mhip_ref_rescue_run", p, rid_end - rid_begin, tech)) return -1;
    if (idx->max_bucket != MAX_BUCKET) { mhip_set_error("mhip_ref_rescue_run needs an index built with mhip_index_build (bucket cap 128), not %d", idx->max_bucket); return -1; }
    if (idx->num_bases != ref->num_bases) { mhip_set_error("mhip_ref_rescue_run: the index was not built from this reference volume"); return -1; }
    for (int r = rid_begin; r < rid_end; ++r)
        if (reads->h_offs[r].size >= RF_RM) {
            mhip_set_error("mhip_ref_rescue_run: read %d has %d letters; mecat2ref's read buffers hold fewer than %d", r, reads->h_offs[r].size, RF_RM);
            return -1;
        }
    return 0;
}

// the two run entry points of technology `tech` (0: DiffAligner behind the rescue candidates, 1: XdropAligner)
int rr_run_dev(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
               const mhip_ref_rescue_params* p, const mhip_ref_result* d_res, int64_t* total_words, int tech) {
    HIPCHK(hipSetDevice(c->device));
    c->rr_n = 0;
    if (rr_check_run(c, idx, ref, reads, rid_begin, rid_end, p, tech)) return -1;
    const int n = rid_end - rid_begin;
    if (!d_res && n > 0) {
        if (c->rx_slots[0] != n * p->maxc) {
            mhip_set_error("mhip_ref_rescue_run_dev: the last mhip_ref_extend_run on this context left %d slots, not %d reads x %d", c->rx_slots[0], n, p->maxc);
            return -1;
        }
        if (scratch_set(c, "rx_res", 0, 0, (void**)&d_res)) return -1;
    }
    return rescue_run(c, idx, ref, reads, rid_begin, rid_end, p, d_res, total_words, tech ? RX_ALIGNER_XDROP : RX_ALIGNER_DIFF);
}

int rr_run_host(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                const mhip_ref_rescue_params* p, const mhip_ref_result* res, int64_t* total_words, int tech) {
    HIPCHK(hipSetDevice(c->device));
    c->rr_n = 0;
    if (rr_check_run(c, idx, ref, reads, rid_begin, rid_end, p, tech)) return -1;
    const int n = rid_end - rid_begin;
    mhip_ref_result* d_res = nullptr;
    if (n > 0) {
        if (c->scratch("rr_res", sizeof(mhip_ref_result) * (size_t)n * p->maxc, (void**)&d_res)) return -1;
        HIPCHK(hipMemcpyAsync(d_res, res, sizeof(mhip_ref_result) * (size_t)n * p->maxc, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));       // (the caller's array is read until here)
    }
    return rescue_run(c, idx, ref, reads, rid_begin, rid_end, p, d_res, total_words, tech ? RX_ALIGNER_XDROP : RX_ALIGNER_DIFF);
}

}  // namespace

extern "C" {

void mhip_ref_rescue_params_default(mhip_ref_rescue_params* p, int tech) {
    p->maxc = 10;          // kDefaultNumCandidates, mecat2ref.cpp:18
    p->round = 0;
    p->num_output = 10;    // kDefaultNumOutput, mecat2ref.cpp:19
    p->tech = tech;
    p->ddfs_cutoff = 0.25;
}

int mhip_ref_rescue_run_dev(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                            const mhip_ref_rescue_params* p, const mhip_ref_result* d_res, int64_t* total_words) {
    return rr_run_dev(c, idx, ref, reads, rid_begin, rid_end, p, d_res, total_words, 0);
}

int mhip_ref_rescue_run(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                        const mhip_ref_rescue_params* p, const mhip_ref_result* res, int64_t* total_words) {
    return rr_run_host(c, idx, ref, reads, rid_begin, rid_end, p, res, total_words, 0);
}

/* nanopore mode: the same stage with the X-drop extension (ref_xextend.hip) behind the rescue candidates */
int mhip_ref_xrescue_run_dev(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                             const mhip_ref_rescue_params* p, const mhip_ref_result* d_res, int64_t* total_words) {
    return rr_run_dev(c, idx, ref, reads, rid_begin, rid_end, p, d_res, total_words, 1);
}

int mhip_ref_xrescue_run(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                         const mhip_ref_rescue_params* p, const mhip_ref_result* res, int64_t* total_words) {
    return rr_run_host(c, idx, ref, reads, rid_begin, rid_end, p, res, total_words, 1);
}

int mhip_ref_rescue_fetch(mhip_ctx* c, int32_t* out_slots, int32_t* out_counts, mhip_ref_candidate* rescue_cands, int32_t* rescue_counts,
                          mhip_ref_result* rescue_res, uint64_t* word_offs, uint32_t* ops_dense) {
    HIPCHK(hipSetDevice(c->device));
    const int n = c->rr_n;
    if (n == 0) { if (word_offs) word_offs[0] = 0; return 0; }
    int32_t *d_os, *d_oc, *d_rcount;
    mhip_ref_candidate* d_cands;
    if (c->scratch("rr_out_slots", 0, (void**)&d_os) || c->scratch("rr_out_counts", 0, (void**)&d_oc) || c->scratch("rr_rcount", 0, (void**)&d_rcount) ||
        c->scratch("rr_cands", 0, (void**)&d_cands))
        return -1;
    HIPCHK(hipMemcpyAsync(out_slots, d_os, sizeof(int32_t) * (size_t)n * 3 * c->rr_num_output, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_counts, d_oc, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(rescue_cands, d_cands, sizeof(mhip_ref_candidate) * (size_t)n * RR_TRIES, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(rescue_counts, d_rcount, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    return ref_extend_fetch(c, 1, rescue_res, word_offs, ops_dense);
}

void mhip_ref_rescue_stats(int64_t out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = g_rescue_stats[i];
}

int mhip_debug_ref_rescue_prep(mhip_ctx* c, const mhip_ref_rescue_params* p, int n, const mhip_ref_result* res, mhip_ref_rescue_state* states) {
    HIPCHK(hipSetDevice(c->device));
    c->rr_n = 0;          // (the hooks write the run's buffers: nothing of a run is left to fetch)
    if (rr_check("mhip_debug_ref_rescue_prep", p, n)) return -1;
    if (n == 0) return 0;
    mhip_ref_result* d_res;
    mhip_ref_rescue_state* d_st;
    if (c->scratch("rr_res", sizeof(mhip_ref_result) * (size_t)n * p->maxc, (void**)&d_res)) return -1;
    if (c->scratch("rr_state", sizeof(mhip_ref_rescue_state) * (size_t)n, (void**)&d_st)) return -1;
    HIPCHK(hipMemcpyAsync(d_res, res, sizeof(mhip_ref_result) * (size_t)n * p->maxc, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "ref_rescue_prep", ref_rescue_prep, (n + RR_BLOCK - 1) / RR_BLOCK, RR_BLOCK, 0, (const mhip_ref_result*)d_res, n, p->maxc, d_st, (int*)nullptr,
           (unsigned int*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(states, d_st, sizeof(mhip_ref_rescue_state) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int mhip_debug_ref_rescue_finish(mhip_ctx* c, const mhip_ref_rescue_params* p, int n, const mhip_ref_result* res, const mhip_ref_rescue_state* states,
                                 const int32_t* rescue_counts, const int32_t* rescue_meta, const mhip_ref_result* rescue_res, int32_t* out_slots,
                                 int32_t* out_counts) {
    HIPCHK(hipSetDevice(c->device));
    c->rr_n = 0;
    if (rr_check("mhip_debug_ref_rescue_finish", p, n)) return -1;
    if (n == 0) return 0;
    for (int i = 0; i < n; ++i) {
        const mhip_ref_rescue_state& s = states[i];
        bool bad = s.naln < 0 || s.naln > p->maxc || s.nres < s.naln || s.nres > p->maxc || rescue_counts[i] < 0 || rescue_counts[i] > RR_TRIES;
        for (int k = 0; !bad && k < s.naln; ++k) bad = s.slot[k] < 0 || s.slot[k] >= p->maxc || s.id[k] < 0 || s.id[k] >= s.nres;
        for (int j = 0; !bad && j < rescue_counts[i]; ++j) {
            const int m = rescue_meta[(size_t)i * RR_TRIES + j];
            bad = (m & 0xff) >= std::min(s.naln, 3) || (m >> 8) < 0 || (m >> 8) > 1;
        }
        if (bad) { mhip_set_error("mhip_debug_ref_rescue_finish: read %d: a state or a rescue list that ref_rescue_prep and the search cannot give", i); return -1; }
    }
    mhip_ref_result *d_res, *d_rres;
    mhip_ref_rescue_state* d_st;
    int32_t *d_cnt, *d_meta, *d_os, *d_oc;
    const size_t no = (size_t)n * 3 * p->num_output;
    if (c->scratch("rr_res", sizeof(mhip_ref_result) * (size_t)n * p->maxc, (void**)&d_res)) return -1;
    if (c->scratch("rr_state", sizeof(mhip_ref_rescue_state) * (size_t)n, (void**)&d_st)) return -1;
    if (c->scratch("rr_rres", sizeof(mhip_ref_result) * (size_t)n * RR_TRIES, (void**)&d_rres)) return -1;
    if (c->scratch("rr_rcount", sizeof(int32_t) * (size_t)n, (void**)&d_cnt)) return -1;
    if (c->scratch("rr_meta", sizeof(int32_t) * (size_t)n * RR_TRIES, (void**)&d_meta)) return -1;
    if (c->scratch("rr_out_slots", sizeof(int32_t) * no, (void**)&d_os)) return -1;
    if (c->scratch("rr_out_counts", sizeof(int32_t) * (size_t)n, (void**)&d_oc)) return -1;
    HIPCHK(hipMemcpyAsync(d_res, res, sizeof(mhip_ref_result) * (size_t)n * p->maxc, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_st, states, sizeof(mhip_ref_rescue_state) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_rres, rescue_res, sizeof(mhip_ref_result) * (size_t)n * RR_TRIES, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_cnt, rescue_counts, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_meta, rescue_meta, sizeof(int32_t) * (size_t)n * RR_TRIES, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "ref_rescue_finish", ref_rescue_finish, (n + RR_BLOCK - 1) / RR_BLOCK, RR_BLOCK, 0, (const mhip_ref_result*)d_res, (const mhip_ref_rescue_state*)d_st,
           (const int32_t*)d_cnt, (const int32_t*)d_meta, (const mhip_ref_result*)d_rres, n, p->maxc, p->num_output, d_os, d_oc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_slots, d_os, sizeof(int32_t) * no, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_counts, d_oc, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
