// seed_cand.hip — the get_candidates replay of the seeding stage and its launcher (seed.hip describes the stage)
#include "seed_defs.h"
#include "seed_replay.h"

#define SWEEP_G 8       // neighbour segments of a sweep whose lists are in flight together

struct CandLds {
    int t_loc[2 * SM + 10];
    int t_seed[2 * SM + 10];
};

// index of segment `seg` in the strand's segment table, or -1
__device__ __forceinline__ int seg_find(const uint32_t* __restrict__ seg_id, int nseg, uint32_t seg) {
    int lo = 0, hi = nseg;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (seg_id[mid] < seg) lo = mid + 1; else hi = mid;
    }
    return (lo < nseg && seg_id[lo] == seg) ? lo : -1;
}

// all-f32 DDF test of find_location (pw_impl.cpp:165,196,222)
__device__ __forceinline__ bool ddf_find(int dloc, int dseed, double cutoff) {
    float r = (float)dloc / ((float)dseed * 10.0f) - 1.0f;
    return (double)fabsf(r) < cutoff;
}

// ddf_find for cutoff == 0.25 (the reference's value in every mode) without the division.  dloc, dseed > 0 are small
// integers, so x = dloc / (10 dseed) is never within a rounding error of 0.75 or 1.25 unless it equals them
// (|x - 1.25| >= 1 / (40 dseed) >= 7.6e-7 for dseed < 32768, half an f32 ulp there is 6e-8): q = RN(x) satisfies
// 0.75 < q < 1.25 exactly when x does; q - 1 is exact for q in [0.5, 2] (Sterbenz) and |RN(q - 1)| >= 0.5 outside.
__device__ __forceinline__ bool ddf_find_quarter(int dloc, int dseed) {        // |dseed| < 2^15: 24-bit multiplies
    return (int)(2 * dloc > __mul24(15, dseed)) & (int)(2 * dloc < __mul24(25, dseed));
}

// lane `l` (wave-uniform) of `old` replaced by the wave-uniform value `v`
__device__ __forceinline__ int write_lane(int v, int l, int old) {
    // two scalar operands exceed the constant bus: the lane select goes through m0 (the compiler sets m0 anew before each of its own uses)
    asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(old) : "s"(v), "s"(l));
    return old;
}

// one wave per read: F strand then R strand into one top-MAXC list kept in LDS (12 ints per entry)
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(7, 7))) void seed_cand(SeedArrays AF, SeedArrays AB, const mhip_offset_t* __restrict__ ref_offs, const uint32_t* __restrict__ ref_blk, int ref_nreads,
                                                  int ref_start_id, const mhip_offset_t* __restrict__ roffs, ReadSel sel, int ib,
                                                  int reads_start_id, mhip_params P, mhip_candidate* __restrict__ out,
                                                  int32_t* __restrict__ out_counts, unsigned long long* __restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int lane = lane_id();
    // the batch's reads last-first: a read's subjects are the reads with lower ids, so the longest waves start first
    const int r = (int)gridDim.x - 1 - (int)blockIdx.x;
    // the list: [maxc][12] in LDS; a list too long for that (-n above 1024: the reference takes any positive -n, pw_options.cpp:9) is
    // built in place in the read's slice of the output table — the same code on global memory, read past the L1 (the wave reads its
    // own earlier stores)
    const bool big = P.maxc > MAXC_LDS;
    int* clist = big ? (int*)(out + (size_t)r * P.maxc) : smem;
    CandLds* T = (CandLds*)(smem + (big ? 0 : P.maxc * 12));
    auto cl_ld = [&](int i) -> int { return big ? __hip_atomic_load(clist + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : clist[i]; };
    auto cl_st = [&](int i, int v) { if (big) __hip_atomic_store(clist + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else clist[i] = v; };
    const int rid = sel_rid(sel, ib + r);
    const int read_id = rid + reads_start_id;
    const int read_size = roffs[rid].size;
    const int MAXC = P.maxc;
    const double cutoff = P.ddfs_cutoff;
    int ncand = 0;

    for (int strand = 0; strand < 2; ++strand) {
        const int s = 2 * r + strand;
        const SeedArrays& A = AF.fused[s] ? AF : AB;          // the strand's tables: from seed_strand or from the kernel chain
        const uint64_t hb = A.hit_base[s];
        const int nseg = (int)A.nseg[s];
        const int ng = (int)A.ngated[s];
        if (A.strand_hits[s] == 0) continue;
        uint32_t* ent = A.ent + hb;
        uint32_t* fin = A.ent_fin + hb;
        const uint32_t* seg_id = A.seg_id + hb;
        const uint32_t* seg_start = A.seg_start + hb;
        int32_t* seg_score = A.seg_score + hb;
        const uint32_t* gated = A.gated + hb;
#define SEG_LIST(g) (((seg_score[g] & OVF_FLAG) ? fin : ent) + seg_start[g])
#define SEG_SCORE(g) (seg_score[g] & ~OVF_FLAG)
#define SET_SCORE(g, v) seg_score[g] = (seg_score[g] & OVF_FLAG) | (v)
#define HAS_LEFT 0x40000000           // (a segment id has 21 bits)

        // The walk is a chain of dependent loads from HBM (gated -> ids / starts -> scores -> lists), and its time is the number of
        // round trips.  The gated list is taken in chunks of 64: lane j holds entry gi - gi % 64 + j — the immutable part of its
        // record (table index, segment id with "the table's entry before it is the segment before it" in bit 30, the two list
        // starts) and a copy of the two scores an iteration starts from.  The scores are the only part an earlier iteration changes
        // (the sweeps and the self-hit scrub zero or lower them): the copy is loaded anew, one load per lane, behind every iteration
        // that wrote one, so an entry that was zeroed costs its iteration no load at all, and a live one starts with its lists.
        int gv = 0, segv = 0, scv = 0, scm1v = 0;
        uint32_t stv = 0, stm1v = 0;
        bool stale = true;
        for (int gi = 0; gi < ng; ++gi) {
            const int gj = gi & 63;
            if (gj == 0) {
                gv = segv = 0;
                stv = stm1v = 0;
                if (gi + lane < ng) {
                    gv = (int)gated[gi + lane];
                    segv = (int)seg_id[gv];
                    stv = seg_start[gv];
                    const int segm1 = gv > 0 ? (int)seg_id[gv - 1] : -1;
                    if (segv > 0 && gv > 0 && segm1 == segv - 1) { segv |= HAS_LEFT; stm1v = seg_start[gv - 1]; }
                }
                stale = true;
            }
            if (stale) {
                scv = scm1v = 0;
                if (gi - gj + lane < ng) {
                    scv = seg_score[gv];
                    if (segv & HAS_LEFT) scm1v = seg_score[gv - 1];
                }
                stale = false;
            }
#ifdef CAND_STATS
            if (lane == 0) atomicAdd(&counters[9], 1ull);
#endif
            const int raw_g = __builtin_amdgcn_readlane(scv, gj);
            int s_k = raw_g & ~OVF_FLAG;
            if (s_k == 0) continue;
#ifdef CAND_STATS
            if (lane == 0) atomicAdd(&counters[10], 1ull);
#endif
            const int g = __builtin_amdgcn_readlane(gv, gj), seg = __builtin_amdgcn_readlane(segv, gj) & ~HAS_LEFT;
            const uint32_t st_g = (uint32_t)__builtin_amdgcn_readlane((int)stv, gj), st_gm1 = (uint32_t)__builtin_amdgcn_readlane((int)stm1v, gj);
            const int raw_gm1 = __builtin_amdgcn_readlane(scm1v, gj);        // 0 without a left neighbour
            const int loc = raw_gm1 & ~OVF_FLAG;
            int start_loc = seg * ZV;
            if (loc > 0) start_loc = (seg - 1) * ZV;
            const int n1 = loc > 0 ? min(loc, SM) : 0, n2 = min(s_k, SM);
            const int k = n1 + n2;
            const uint32_t* list_g = ((raw_g & OVF_FLAG) ? fin : ent) + st_g;
            const uint32_t* list_gm1 = ((raw_gm1 & OVF_FLAG) ? fin : ent) + st_gm1;
            __syncthreads();
            for (int i = lane; i < k; i += 64) {
                uint32_t e = i < n1 ? list_gm1[i] : list_g[i - n1];
                T->t_loc[i] = ent_loc(e) + ((i >= n1 && loc > 0) ? ZV : 0);
                T->t_seed[i] = ent_seed(e);
            }
            __syncthreads();
            // ---- find_location (pw_impl.cpp:161-239): lane owns entries i0 = lane and i1 = lane + 64
            const int i0 = lane, i1 = lane + 64;
            const int l0 = i0 < k ? T->t_loc[i0] : 0, d0 = i0 < k ? T->t_seed[i0] : 0;
            const int l1 = i1 < k ? T->t_loc[i1] : 0, d1 = i1 < k ? T->t_seed[i1] : 0;
            int temp0 = d0, temp1 = d1, sc0 = 0, sc1 = 0;
            // entries 64.. exist only when both lists are long (k <= 80); most segment pairs fit one entry per lane
            const int k0 = min(k, 64);
            // Branch-free: every condition is evaluated for every lane and combined with &; the votes an entry receives from
            // the entries before it go through a lane write (each j is written once) and are added after the loops.
            int in0 = 0, in1 = 0;
            auto vote_loops = [&](auto ddf) {
                for (int j = 1; j < k0; ++j) {
                    const int lj = __builtin_amdgcn_readlane(l0, j), dj = __builtin_amdgcn_readlane(d0, j);     // entry j lives in lane j
                    const int ds = dj - d0, dl = lj - l0;
                    const bool v0 = (i0 < j) & (temp0 != dj) & (ds > 0) & (dl > 0) & (dl < read_size) & ddf(dl, ds);
                    sc0 += v0 ? 1 : 0;
                    temp0 = v0 ? dj : temp0;
                    in0 = write_lane(__popcll(__builtin_amdgcn_ballot_w64(v0)), j, in0);
                }
                for (int j = 64; j < k; ++j) {
                    const int lj = __builtin_amdgcn_readlane(l1, j - 64), dj = __builtin_amdgcn_readlane(d1, j - 64);
                    const int ds0 = dj - d0, dl0 = lj - l0, ds1 = dj - d1, dl1 = lj - l1;
                    const bool v0 = (temp0 != dj) & (ds0 > 0) & (dl0 > 0) & (dl0 < read_size) & ddf(dl0, ds0);
                    const bool v1 = (i1 < j) & (temp1 != dj) & (ds1 > 0) & (dl1 > 0) & (dl1 < read_size) & ddf(dl1, ds1);
                    sc0 += v0 ? 1 : 0;
                    temp0 = v0 ? dj : temp0;
                    sc1 += v1 ? 1 : 0;
                    temp1 = v1 ? dj : temp1;
                    in1 = write_lane(__popcll(__builtin_amdgcn_ballot_w64(v0)) + __popcll(__builtin_amdgcn_ballot_w64(v1)), j - 64, in1);
                }
            };
            if (cutoff == 0.25) vote_loops([](int dloc, int dseed) { return ddf_find_quarter(dloc, dseed); });
            else vote_loops([&](int dloc, int dseed) { return (dloc > 0) & (dseed > 0) & ddf_find(dloc, dseed, cutoff); });
            sc0 += in0;
            sc1 += in1;
            int mv = max(i0 < k ? sc0 : -1, i1 < k ? sc1 : -1);
            for (int o = 32; o > 0; o >>= 1) mv = max(mv, __shfl_xor(mv, o));
            const int maxval = mv;
#ifdef CAND_STATS
            if (lane == 0 && maxval < 5) atomicAdd(&counters[11], 1ull);
            if (lane == 0) atomicAdd(&counters[12], (unsigned long long)k);
#endif
            if (maxval < 5) continue;
            const uint64_t eq0 = __ballot(i0 < k && sc0 == maxval), eq1 = __ballot(i1 < k && sc1 == maxval);
            const int maxi = eq0 ? __ffsll((unsigned long long)eq0) - 1 : 64 + __ffsll((unsigned long long)eq1) - 1;
            const int rep = __popcll(eq0) + __popcll(eq1) - 1;
            int rep_loc;
            if (rep == maxval) {
                rep_loc = maxi;
            } else {
                const int lm = T->t_loc[maxi], dm = T->t_seed[maxi];
                // selected = DDF-consistent with maxi (before: "< read_len", after: "<= read_len"), plus maxi itself
                bool q0 = false, q1 = false;
                if (i0 < k) {
                    if (i0 < maxi) q0 = dm - d0 > 0 && lm - l0 > 0 && lm - l0 < read_size && ddf_find(lm - l0, dm - d0, cutoff);
                    else if (i0 == maxi) q0 = true;
                    else q0 = d0 - dm > 0 && l0 - lm > 0 && l0 - lm <= read_size && ddf_find(l0 - lm, d0 - dm, cutoff);
                }
                if (i1 < k) {
                    if (i1 < maxi) q1 = dm - d1 > 0 && lm - l1 > 0 && lm - l1 < read_size && ddf_find(lm - l1, dm - d1, cutoff);
                    else if (i1 == maxi) q1 = true;
                    else q1 = d1 - dm > 0 && l1 - lm > 0 && l1 - lm <= read_size && ddf_find(l1 - lm, d1 - dm, cutoff);
                }
                const uint64_t s0m = __ballot(q0), s1m = __ballot(q1);
                const uint64_t z0 = __ballot(q0 && l0 != 0), z1 = __ballot(q1 && l1 != 0);
                // loc[0] == 0 doubles as "unset" (pw_impl.cpp:198,211,224): first selected entry with a non-zero
                // location wins; if every selected location is 0 the last selected entry wins
                if (z0) rep_loc = __ffsll((unsigned long long)z0) - 1;
                else if (z1) rep_loc = 64 + __ffsll((unsigned long long)z1) - 1;
                else if (s1m) rep_loc = 64 + (63 - __clzll((unsigned long long)s1m));
                else rep_loc = 63 - __clzll((unsigned long long)s0m);
            }
            const int vote = rep_loc < 64 ? __shfl(sc0, rep_loc) : __shfl(sc1, rep_loc - 64);
            // (one LDS word each, the same in every lane: kept in scalar registers, and the geometry below with them)
            const int loc_seed = __builtin_amdgcn_readfirstlane(T->t_seed[rep_loc]);
            const int loc_list = start_loc + __builtin_amdgcn_readfirstlane(T->t_loc[rep_loc]);
            // the subject lookup's first load, requested ahead of the threshold test (a location is a hit's: inside the volume)
            const int blk_r = loc_list >= 0 ? (int)ref_blk[loc_list >> 10] : 0;
            if (vote < 2 * P.min_kmer_match + 2) continue;
            int sid = read_id_lookup_from(ref_offs, ref_nreads, blk_r, loc_list);
            const int sstart = ref_offs[sid].offset, ssize = ref_offs[sid].size;
            const int send = sstart + ssize + 1;
            sid += ref_start_id;
            if (sid > read_id) continue;
            if (sid == read_id) {
                // scrub the read's own region (pw_impl.cpp:371-383); only loczhi is compacted, seedno is not
                int u_k = sstart / ZV;
                int gg = seg_find(seg_id, nseg, (uint32_t)u_k);
                if (gg >= 0) {
                    const int lim = sstart % ZV, cnt = min(SEG_SCORE(gg), SM);
                    uint32_t* L = SEG_LIST(gg);
                    uint32_t e = lane < cnt ? L[lane] : 0;
                    bool keep = lane < cnt && ent_loc(e) < lim;
                    uint64_t km = __ballot(keep);
                    int dstp = __popcll(km & ((1ull << lane) - 1ull));
                    __syncthreads();
                    if (keep) L[dstp] = (L[dstp] & 0xFFFFu) | (e & 0xFFFF0000u);
                    __syncthreads();
                    if (lane == 0) SET_SCORE(gg, __popcll(km));
                }
                ++u_k;
                const int kend = send / ZV;
                {
                    // segments strictly between: score = 0
                    int lo = 0, hi = nseg;
                    while (lo < hi) { int mid = (lo + hi) >> 1; if ((int)seg_id[mid] < u_k) lo = mid + 1; else hi = mid; }
                    for (int x = lo + lane; x < nseg && (int)seg_id[x] < kend; x += 64) SET_SCORE(x, 0);
                }
                const int tail_seg = max(u_k, kend);
                gg = seg_find(seg_id, nseg, (uint32_t)tail_seg);
                __syncthreads();
                if (gg >= 0) {
                    const int lim = send % ZV, cnt = min(SEG_SCORE(gg), SM);
                    uint32_t* L = SEG_LIST(gg);
                    uint32_t e = lane < cnt ? L[lane] : 0;
                    bool keep = lane < cnt && ent_loc(e) > lim;
                    uint64_t km = __ballot(keep);
                    int dstp = __popcll(km & ((1ull << lane) - 1ull));
                    __syncthreads();
                    if (keep) L[dstp] = (L[dstp] & 0xFFFFu) | (e & 0xFFFF0000u);
                    __syncthreads();
                    if (lane == 0) SET_SCORE(gg, __popcll(km));
                }
                __syncthreads();
                stale = true;
                continue;
            }
            // ---- geometry (pw_impl.cpp:386-403)
            const int loc2 = (loc_seed - 1) * BC;
            const int left1 = loc_list - sstart + MHIP_KMER_SIZE - 1, right1 = send - loc_list;
            const int left2 = loc2 + MHIP_KMER_SIZE - 1, right2 = read_size - loc2;
            const int num1 = left1 > left2 ? left2 : left1, num2 = right1 > right2 ? right2 : right1;
            if (num1 + num2 < P.min_kmer_dist) continue;
            // ---- neighbour sweeps (pw_impl.cpp:405-438), f64
            int seedcount = 0;
            // A neighbour's test reads its own segment and writes its own score, so the order inside a sweep is free, and the two sweeps
            // go together (seedcount is a sum).  Round c takes 32 neighbours of either side: lane j < 32 owns the left neighbour
            // x = g - 1 - 32 c - j, lane 32 + j the right one x = g + 1 + 32 c + j, and loads its table entry: one round trip for both
            // sides.  The lists of the live ones are then requested SWEEP_G segments at a time, left side first, before the first of
            // them is tested: one more.  A segment's agreeing entries are counted into its owner's lane, and the owners zero the
            // scores at the round's end.
            {
                const int nlb = (num1 + ZV - 1) / ZV, nrb = (num2 + ZV - 1) / ZV;
                const int lowest = max(0, seg - nlb);          // segments seg-1 .. lowest
                const int highest = seg + nrb;                  // segments seg+1 .. highest
                const bool lside = lane < 32;
                uint64_t more = ~0ull;                          // the lanes of a side that may have neighbours left
                for (int c = 0; more; ++c) {
                    const int x = lside ? g - 1 - 32 * c - lane : g + 1 + 32 * c + (lane - 32);
                    int id = -1, raw = 0;
                    uint32_t st = 0;
                    if (((more >> lane) & 1) && x >= 0 && x < nseg) { id = (int)seg_id[x]; raw = seg_score[x]; st = seg_start[x]; }
                    // the table ascends: the neighbours inside a sweep's reach are the first lanes of its side
                    const bool in = id >= 0 && (lside ? id >= lowest : id <= highest);
                    const uint64_t inm = __builtin_amdgcn_ballot_w64(in);
                    more = ((uint32_t)inm == 0xFFFFFFFFu ? 0xFFFFFFFFull : 0ull) | ((uint32_t)(inm >> 32) == 0xFFFFFFFFu ? 0xFFFFFFFF00000000ull : 0ull);
                    const int scnt = min(raw & ~OVF_FLAG, SM);
                    const uint64_t live = __builtin_amdgcn_ballot_w64(in && (raw & ~OVF_FLAG) > 0);
                    int agv = 0;
                    uint64_t m = live;
                    while (m) {
                        uint32_t e[SWEEP_G];
                        uint64_t p = m;
#pragma unroll
                        for (int q = 0; q < SWEEP_G; ++q) {      // (no branch on a slot without a segment: no lane loads)
                            const bool has = p != 0;
                            const int j = has ? __builtin_ctzll(p) : 0;
                            p &= p - 1;
                            const int rj = __builtin_amdgcn_readlane(raw, j);
                            const uint32_t* L = ((rj & OVF_FLAG) ? fin : ent) + (uint32_t)__builtin_amdgcn_readlane((int)st, j);
                            e[q] = 0;
                            if (has && lane < min(rj & ~OVF_FLAG, SM)) e[q] = L[lane];
                        }
#pragma unroll
                        for (int q = 0; q < SWEEP_G; ++q) {
                            if (m) {
                                const int j = __builtin_ctzll(m);
                                m &= m - 1;
                                const int sl = __builtin_amdgcn_readlane(id, j) * ZV, sc = __builtin_amdgcn_readlane(scnt, j);
                                const int l = ent_loc(e[q]), sd = ent_seed(e[q]);
                                const int dl = j < 32 ? loc_list - sl - l : sl + l - loc_list;
                                const int ds = j < 32 ? loc_seed - sd : sd - loc_seed;
                                const bool ok = lane < sc && fabs((double)dl / ((double)(ds * BC) * 1.0) - 1.0) < cutoff;
                                const int agree = __popcll(__builtin_amdgcn_ballot_w64(ok));
                                seedcount += agree;
                                agv = write_lane(agree, j, agv);
                            }
                        }
                    }
                    const bool zero = ((live >> lane) & 1) && agv * 1.0 / scnt > 0.4;
                    if (zero) seg_score[x] = raw & OVF_FLAG;
                    stale |= __builtin_amdgcn_ballot_w64(zero) != 0;
                }
                if (stale) __syncthreads();
            }
            const int cscore = vote + seedcount;
            // ---- stable insertion into the descending top-MAXC list (pw_impl.cpp:442-455)
            int ge = 0;
            for (int i = lane; i < ncand; i += 64) ge += cl_ld(i * 12 + 6) >= cscore ? 1 : 0;
            for (int o = 32; o > 0; o >>= 1) ge += __shfl_xor(ge, o);
            const int pos = ge;                                  // == high + 1
            const int last_src = (ncand < MAXC) ? ncand - 1 : ncand - 2;
            __syncthreads();
            for (int top = last_src; top >= pos; top -= 64) {
                const int i = top - lane;
                int v[12];
                if (i >= pos) {
#pragma unroll
                    for (int q = 0; q < 12; ++q) v[q] = cl_ld(i * 12 + q);
                }
                __syncthreads();
                if (i >= pos) {
#pragma unroll
                    for (int q = 0; q < 12; ++q) cl_st((i + 1) * 12 + q, v[q]);
                }
                __syncthreads();
            }
            if (pos < MAXC && lane == 0) {
                const int cv[12] = {loc_list - sstart, loc2, left1, left2, right1, right2, cscore, num1, num2, sid, sstart, strand};
#pragma unroll
                for (int q = 0; q < 12; ++q) cl_st(pos * 12 + q, cv[q]);
            }
            if (ncand < MAXC) ++ncand;
            __syncthreads();
        }
#undef SEG_LIST
#undef SEG_SCORE
#undef SET_SCORE
#undef HAS_LEFT
    }
    __syncthreads();
    int* o = (int*)(out + (size_t)r * MAXC);
    if (!big)
        for (int i = lane; i < ncand * 12; i += 64) o[i] = clist[i];
    if (lane == 0) {
        out_counts[r] = ncand;
        atomicAdd(&counters[2], (unsigned long long)ncand);
    }
}

// ------------------------------------------------------------------------------------------------ launcher
int seed_run_cand(const SeedBatch& b) {
    mhip_ctx* c = b.c;
    const mhip_params* P = b.P;
    // LDS: the top-MAXC list while it fits (seed_cand builds a longer one in the output table) and the vote lists
    const size_t lds = sizeof(int) * 12 * (size_t)(P->maxc > MAXC_LDS ? 0 : P->maxc) + sizeof(CandLds);
    LAUNCH(c, "seed_cand", seed_cand, b.nr, WAVE, lds, b.F, b.B, (const mhip_offset_t*)b.ref->d_offs, (const uint32_t*)b.ref->d_blk2read,
           b.ref->num_reads, b.ref->start_read_id, (const mhip_offset_t*)b.reads->d_offs, b.sel, b.ib, b.reads->start_read_id, *P, b.d_out,
           b.d_counts, (unsigned long long*)c->d_counters);
    return 0;
}
