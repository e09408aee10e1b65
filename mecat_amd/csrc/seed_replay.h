// seed_replay.h — device helpers of the seeding stage that more than one kernel family calls (seed_defs.h lists the families):
//   sweep_reach                    seed_filter, seed_filter_wide, seed_strand
//   ddf_insert, replay_overflow    seed_build, seed_strand
//   read_id_lookup                 through subjects_all_higher seed_build and seed_strand
//   read_id_lookup_from            seed_cand
#pragma once

#include "seed_defs.h"

// sweeps of get_candidates reach ceil(num / ZV) segments, num <= read length + 12 (pw_impl.cpp:388-425); +1 for seg - 1
__device__ __forceinline__ int sweep_reach(int L) { return (L + MHIP_KMER_SIZE - 1 + ZV - 1) / ZV + 1; }

// f32 divide, f64 compare: the DDF test of insert_loc (pw_impl.cpp:135)
__device__ __forceinline__ bool ddf_insert(int dloc, int dseed, double cutoff) {
    float r = (float)dloc / ((float)dseed * 10.0f);
    return fabs((double)r - 1.0) < cutoff;
}

// insert_loc replay for one overflowed segment by one wave.  Events e = 40.. c-1 (0-based) arrive one by one.
// lane i (< 40) holds list entry i.  Writes the final 40 entries to fin[] and the score after each event to esc[].
//
// While the 40-entry list is one exact chain (strictly increasing seed numbers, loc advancing by BC per seed from entry to
// entry) an event that continues the chain after the last entry passes every pair test: the minimum is SM and the event just
// replaces the last entry (pw_impl.cpp:121-159 with every score equal).  Runs of such events are skipped in one step — a read
// against its own copy in the volume is the common overflow and is such a chain from end to end, bar the odd random hit,
// which is looked at, thrown out again, and leaves the list the chain it was.
__device__ void replay_overflow(const uint32_t* __restrict__ ev, int c, uint32_t* __restrict__ fin, uint16_t* __restrict__ esc,
                                double cutoff, int* score_out) {
    const int lane = lane_id();
    int loc = 0, seed = 0;
    if (lane < SM) { const uint32_t e0 = ev[lane]; loc = ent_loc(e0); seed = ent_seed(e0); }
    if (lane < SM) esc[lane] = (uint16_t)(lane + 1);
    int score = SM;
    int e = SM;
    auto is_chain = [&]() {
        const int nl = __shfl_down(loc, 1), ns = __shfl_down(seed, 1);
        return (bool)__all(lane >= SM - 1 || (ns - seed > 0 && nl - loc == (ns - seed) * BC));
    };
    bool chain = is_chain();
    while (e < c) {
        if (chain) {
            const int lloc = __builtin_amdgcn_readlane(loc, SM - 1), lseed = __builtin_amdgcn_readlane(seed, SM - 1);
            int nb = c;                              // first event that does not continue the chain
            for (int i0 = e; i0 < c && nb == c; i0 += 64) {
                const int i = i0 + lane;
                bool bad = false;
                if (i < c) {
                    const uint32_t b = ev[i];
                    int pl = lloc, ps = lseed;
                    if (i > e) { const uint32_t a = ev[i - 1]; pl = ent_loc(a); ps = ent_seed(a); }
                    const int ds = ent_seed(b) - ps, dl = ent_loc(b) - pl;
                    bad = !(ds > 0 && dl == ds * BC);
                }
                const unsigned long long bm = __ballot(bad);
                if (bm) nb = i0 + __builtin_ctzll(bm);
            }
            if (nb > e) {
                for (int x = e + lane; x < nb; x += 64) esc[x] = (uint16_t)(score + (x - e) + 1);
                score += nb - e;
                if (lane == SM - 1) { const uint32_t le = ev[nb - 1]; loc = ent_loc(le); seed = ent_seed(le); }
                e = nb;
                if (e >= c) break;
            }
        }
        const uint32_t ne = ev[e];
        const int nloc = ent_loc(ne), nseed = ent_seed(ne);
        ++score;   // loc = ++spr->score (pw_impl.cpp:267)
        // element 40 of the 41-entry working list is the new seed
        const int myloc = lane < SM ? loc : nloc, myseed = lane < SM ? seed : nseed;
        int sc = 0;
        for (int i = 0; i < SM; ++i) {
            const int li = __builtin_amdgcn_readlane(myloc, i), si = __builtin_amdgcn_readlane(myseed, i);      // entry i lives in lane i
            const bool pass = lane > i && lane <= SM && myseed - si > 0 && myloc - li > 0 && ddf_insert(myloc - li, myseed - si, cutoff);
            const uint64_t b = __ballot(pass);
            sc += pass ? 1 : 0;
            if (lane == i) sc += __popcll(b);
        }
        const int v = lane <= SM ? sc : 0x7fffffff;
        int m = v;
        for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
        const int minval = m;
        const int mini = __ffsll((unsigned long long)__ballot(v == m)) - 1;   // first index holding the minimum
        if (minval == SM) {
            if (lane == SM - 1) { loc = nloc; seed = nseed; }
        } else if (minval < SM && mini < SM) {
            // delete entry mini, shift left, append the new one
            const int sl = __shfl_down(myloc, 1), ss = __shfl_down(myseed, 1);
            if (lane >= mini && lane < SM) { loc = sl; seed = ss; }
            --score;
        }
        if (lane == 0) esc[e] = (uint16_t)score;
        ++e;
        chain = is_chain();
    }
    if (lane < SM) fin[lane] = ((uint32_t)loc << 16) | ((uint32_t)seed & 0xFFFFu);
    *score_out = score;
}

// get_read_id_from_offset_list (common/split_database.cpp:15-35), literally
__device__ __forceinline__ int read_id_from_offset(const mhip_offset_t* __restrict__ a, int n, int offset) {
    int left = 0, right = n - 1, mid = (left + right) / 2;
    if (a[right].offset < offset) return right;
    while (left <= right) {
        int o = a[mid].offset, z = a[mid].size;
        if (o <= offset && o + z > offset) return mid;
        if (o + z <= offset) left = mid + 1;
        else right = mid - 1;
        mid = (left + right) / 2;
    }
    return mid;
}

// The same answer from the volume's block table for every position inside a read (the only positions a k-mer hit can have):
// entry b is the read holding base 1024 b, so the read of `offset` is that one or one of the next few.  Anything else (a pad
// base, the "unset" location 0 of find_location landing between reads) takes the literal search.
__device__ __forceinline__ int read_id_lookup(const mhip_offset_t* __restrict__ a, int n, const uint32_t* __restrict__ blk, int offset) {
    if (offset >= 0) {
        int r = (int)blk[offset >> 10];
        while (r + 1 < n && a[r].offset + a[r].size <= offset) ++r;
        const int o = a[r].offset, z = a[r].size;
        if (o <= offset && o + z > offset) return r;
    }
    return read_id_from_offset(a, n, offset);
}

// read_id_lookup with its first load made by the caller: r = blk[offset >> 10] (any value where offset < 0)
__device__ __forceinline__ int read_id_lookup_from(const mhip_offset_t* __restrict__ a, int n, int r, int offset) {
    if (offset >= 0) {
        while (r + 1 < n && a[r].offset + a[r].size <= offset) ++r;
        const int o = a[r].offset, z = a[r].size;
        if (o <= offset && o + z > offset) return r;
    }
    return read_id_from_offset(a, n, offset);
}

// every location find_location can return for segment `seg` (with its left neighbour) lies at or behind the start of segment
// seg - 1, and the read lookup is monotone in the position (a pad base belongs to the read before it).  own_end = the first position
// behind the query read's own copy and its pad, when the query volume is the reference volume: no lookup needed then.
__device__ __forceinline__ bool subjects_all_higher(const RefReads& R, uint32_t seg, int rid, int own_end) {
    const int lo = (int)((seg > 0 ? seg - 1u : 0u) * (uint32_t)ZV);
    if (R.same_volume) return lo >= own_end;
    return read_id_lookup(R.offs, R.nreads, R.blk, lo) + R.start_id > rid + R.reads_start_id;
}
