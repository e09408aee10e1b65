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
// Parity: tests/test_gpu_ref_seed.py against tests/golden/ref_cand.npz (recorded from the unmodified mecat2ref) and tests/ref_cand_ref.py.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

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

namespace {

struct RefWaveLds {
    int tl[64], ts[64], tsc[64];     // find_location's lists (at most 2 * 20 entries) / insert_loc's 21
    mhip_ref_candidate cand[RF_MAXC];
};

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
template <bool SUB_F64>
__device__ __forceinline__ void rf_vote(RefWaveLds& S, int n, int lane, float bc, double cutoff, int dist_cap) {
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
    vshort* pool = pool_all + gw * (size_t)pcap * RF_REC;                  // pcap records; record 0 = the untouched record
    volatile uint32_t* dir = dir_all + gw * (size_t)(nseg + 8);
    int* ilist = ilist_all + gw * (size_t)pcap;
    volatile short* iscore = iscore_all + gw * (size_t)pcap;
    volatile int* slotseg = slotseg_all + gw * (size_t)pcap;
    const unsigned long long below = (1ull << lane) - 1ull;
    auto rec = [&](int seg) { return pool + (size_t)dir[seg] * RF_REC; };
    // records [0, hw) of the pool have been initialised and are in the untouched state
    int hw = hw_all[gw];
    auto init_records = [&](int from, int to) {
        for (int r = from; r < to; ++r) {
            vshort* q = pool + (size_t)r * RF_REC;
            if (lane < RF_REC - 2) q[lane] = 0;
            if (lane == 0) rf_set_index(q, -1);
        }
    };
    if (hw == 0) { init_records(0, 1); hw = 1; }
    int nslots = 1;                                                      // records handed out to the strand in hand: [1, nslots)
    rf_sync();

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
            // ---- seeding (:417-453).  Bucket bounds two steps ahead and first positions one step ahead, as in asm_seed.hip.
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
                    const bool fresh_rec = head && dir[seg] == 0u;
                    const unsigned long long fm = __ballot(fresh_rec);
                    if (fm && nslots + (int)__popcll(fm) > pcap) { ovf = true; break; }
                    if (fm) {
                        const int nnew = (int)__popcll(fm);
                        if (nslots + nnew > hw) {
                            init_records(hw, nslots + nnew);
                            hw = nslots + nnew;
                            rf_sync();
                        }
                        if (fresh_rec) {
                            const int sl = nslots + (int)__popcll(fm & below);
                            dir[seg] = (uint32_t)sl;
                            slotseg[sl] = seg;
                        }
                        nslots += nnew;
                    }
                    if (head) {
                        vshort* r = rec(seg);
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
                        vshort* r = rec(__shfl(seg, src));
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
                    if (ev) idx = rf_index(rec(seg));
                    const unsigned long long fresh = __ballot(ev && idx == -1);
                    if (ev) {
                        const int sk = seg > 0 ? newscore + (int)rec(seg - 1)[R_SCORE] : newscore;      // :438-439
                        if (idx == -1) {
                            const int t = touched + (int)__popcll(fresh & below);
                            ilist[t] = seg;
                            iscore[t] = (short)sk;
                            rf_set_index(rec(seg), t);
                        } else iscore[idx] = (short)sk;
                    }
                    touched += (int)__popcll(fresh);
                    rf_sync();
                }
                if (ovf) break;
                s0 = n0; s1 = n1; pfirst = pnext;
                n0 = m0; n1 = m1;
            }
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
                int flag = 0, rep_loc = 0, loc0 = 0, loc1 = 0;
                {
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
                }
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
            // ---- the strand is done (or given up): its records go back to the untouched state (one contiguous stretch of the pool) and their
            // segments' directory entries to 0
            {
                volatile uint32_t* w = (volatile uint32_t*)(pool + RF_REC);         // (RF_REC shorts = 22 words per record)
                const int nw = (nslots - 1) * (RF_REC / 2);
                for (int j = lane; j < nw; j += 64) w[j] = (j % (RF_REC / 2)) == (RF_REC / 2 - 1) ? 0xffffffffu : 0u;
                for (int sl = 1 + lane; sl < nslots; sl += 64) dir[slotseg[sl]] = 0u;
                nslots = 1;
            }
            rf_sync();
        }
        if (ovf) ncand = 0;
        for (int j = lane; j < ncand; j += 64) out[uo * (size_t)maxc + j] = S.cand[j];
        if (lane == 0) {
            out_counts[uo] = ovf ? -1 : ncand;
            atomicMax(cursor + 4, (unsigned int)hw);
            if (ovf) atomicAdd(cursor + 5, 1u);
        }
        rf_sync();
    }
    if (lane == 0) hw_all[gw] = hw;
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
    // One directory + record pool per resident wave, 12 waves per CU (the kernel's registers allow 3 per SIMD), fewer when they would
    // take more than half of the free memory.  MECAT_REF_POOL overrides the pool's records (the test of the second launch makes it small).
    const char* pe = getenv("MECAT_REF_POOL");
    const int pcap = std::min(nseg + 1, std::max(8, pe && atoi(pe) > 0 ? atoi(pe) : RF_POOL));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t rec_bytes = RF_REC * sizeof(short) + sizeof(int) + sizeof(short) + sizeof(int);
    const size_t per_wave = (size_t)pcap * rec_bytes + (size_t)(nseg + 8) * sizeof(uint32_t);
    const size_t max_waves = (size_t)c->num_cus * 12;
    size_t waves = std::min<size_t>(max_waves, std::max<size_t>(1, free_b / 2 / per_wave));
    waves = std::min<size_t>(waves, (size_t)n);
    const unsigned grid = (unsigned)((waves + RF_WAVES - 1) / RF_WAVES);
    waves = (size_t)grid * RF_WAVES;
    short *d_pool, *d_iscore;
    uint32_t* d_dir;
    int *d_ilist, *d_slotseg, *d_hw;
    unsigned int* d_cur;
    if (c->scratch("rf_pool", sizeof(short) * waves * (size_t)pcap * RF_REC, (void**)&d_pool)) return -1;
    if (c->scratch("rf_dir", sizeof(uint32_t) * waves * (size_t)(nseg + 8), (void**)&d_dir)) return -1;
    if (c->scratch("rf_hw", sizeof(int) * waves, (void**)&d_hw)) return -1;
    if (c->scratch("rf_ilist", sizeof(int) * waves * (size_t)pcap, (void**)&d_ilist)) return -1;
    if (c->scratch("rf_iscore", sizeof(short) * waves * (size_t)pcap, (void**)&d_iscore)) return -1;
    if (c->scratch("rf_slotseg", sizeof(int) * waves * (size_t)pcap, (void**)&d_slotseg)) return -1;
    if (c->scratch("rf_cursor", 64, (void**)&d_cur)) return -1;
    HIPCHK(hipMemsetAsync(d_dir, 0, sizeof(uint32_t) * waves * (size_t)(nseg + 8), c->stream));
    HIPCHK(hipMemsetAsync(d_hw, 0, sizeof(int) * waves, c->stream));        // (the pools count as uninitialised: records are set up as they are handed out)
    HIPCHK(hipMemsetAsync(d_cur, 0, 64, c->stream));
    LAUNCH(c, "ref_seed", ref_seed, grid, RF_BLOCK, 0, (const uint32_t*)idx->d_starts, (const int32_t*)idx->d_offsets, (const uint32_t*)reads->d_pac,
           (const uint32_t*)reads->d_npac, (const mhip_offset_t*)reads->d_offs, rid_begin, n, (const int*)nullptr, d_pool, d_dir, d_hw, d_ilist, d_iscore, d_slotseg,
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
        const int full = nseg + 1;
        size_t w2 = std::min<size_t>(std::min<size_t>(waves, redo.size()), std::max<size_t>(1, free_b / 4 / ((size_t)full * rec_bytes)));
        const unsigned grid2 = (unsigned)((w2 + RF_WAVES - 1) / RF_WAVES);
        w2 = (size_t)grid2 * RF_WAVES;
        if (w2 > waves) { mhip_set_error("ref_seed: no room for the worst-case pools of %zu reads", redo.size()); return -1; }
        short *d_pool2, *d_iscore2;
        int *d_ilist2, *d_slotseg2, *d_redo, *d_hw2;
        if (c->scratch("rf_pool_full", sizeof(short) * w2 * (size_t)full * RF_REC, (void**)&d_pool2)) return -1;
        if (c->scratch("rf_ilist_full", sizeof(int) * w2 * (size_t)full, (void**)&d_ilist2)) return -1;
        if (c->scratch("rf_iscore_full", sizeof(short) * w2 * (size_t)full, (void**)&d_iscore2)) return -1;
        if (c->scratch("rf_slotseg_full", sizeof(int) * w2 * (size_t)full, (void**)&d_slotseg2)) return -1;
        if (c->scratch("rf_hw_full", sizeof(int) * w2, (void**)&d_hw2)) return -1;
        if (c->scratch("rf_redo", sizeof(int) * redo.size(), (void**)&d_redo)) return -1;
        HIPCHK(hipMemsetAsync(d_hw2, 0, sizeof(int) * w2, c->stream));
        HIPCHK(hipMemsetAsync(d_cur, 0, 64, c->stream));
        HIPCHK(hipMemcpyAsync(d_redo, redo.data(), sizeof(int) * redo.size(), hipMemcpyHostToDevice, c->stream));
        LAUNCH(c, "ref_seed_full", ref_seed, grid2, RF_BLOCK, 0, (const uint32_t*)idx->d_starts, (const int32_t*)idx->d_offsets, (const uint32_t*)reads->d_pac,
               (const uint32_t*)reads->d_npac, (const mhip_offset_t*)reads->d_offs, rid_begin, (int)redo.size(), (const int*)d_redo, d_pool2, d_dir, d_hw2, d_ilist2,
               d_iscore2, d_slotseg2, nseg, full, Z, p->round, gate, p->ddfs_cutoff, ref->num_bases, p->maxc, d_cur, d_out, d_cnt);
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
