// cns_plan.hip — mecat2cns' consensus plan, computed on the device from the consensus tables while they are still in device memory:
// which stretches of a template will be corrected (segments) and which windows between two matching positions go to the POA.
// It is the part of consensus_one_read_can_* behind the table that reads nothing but the table:
//
//   effective ranges   get_effective_ranges, mecat2cns/mecat_correction.cpp:118-153 (PacBio, :445-447); the whole read for nanopore
//                      (:509) — host code, cns_ranges.h: at most 100 ranges per template, from records the accept replay holds anyway
//   segments           consensus_worker, :203-239: inside every effective range [L, R), in order, a maximal run of positions with
//                      mat_cnt + ins_cnt >= min_cov (:225-227; the counts as unsigned bytes, summed as int: up to 200) is a segment when
//                      `end - beg >= 0.95 * min_size` (:228, a compare in double: handed to the kernels as the smallest integer that
//                      satisfies it, cns_plan_min_run).  A run never crosses from one range into the next (:221-223 restart at L).
//   windows            meap_consensus_one_segment, :81-108: anchors are the positions whose ident has FMAT (:91, :96); positions in front
//                      of the first anchor belong to nothing (:91); from an anchor i to the next anchor j (or the segment's end) the
//                      window (sb = i, se = j) needs refinement when some k in [i, j) has UNDS or FDEL (:98-100), i included, and
//                      meap_cns_one_indel gets mat_cnt + ins_cnt of position i as its min_cov (:103) — `cov` here.
//
// Formulation (every decision is taken by the lane that sits on the position where a run / a window ENDS, from ballots of the step and
// a few wave-uniform values carried from step to step; no atomics: a record's place is a popcount prefix, so the output order is fixed):
//   cns_plan_segments  one WAVE per template, 64 positions per step, one 32-bit word per lane.  m = ballot(cov >= min_cov).  A run ends
//                      in front of lane l when bit l is clear and bit l - 1 (lane 0: `open`, carried) is set; it began behind the
//                      highest clear bit below l, or at the carried start.  The loop runs to position R INCLUSIVE, so that the range's
//                      end is a lane like any other (out of range: bit clear).  Accepted runs go to the template's slot area (capacity
//                      (R - L) / min_run + 1 per range, prefix-summed on the host), rank = popcount of the accept mask below the lane.
//   cns_plan_scan      exclusive prefix sums of 32-bit counts in 64 bits (one block; the counts are per template / per segment)
//   cns_plan_compact   slot areas -> one dense segment array
//   cns_plan_windows   one WAVE per segment, two instantiations of the same walk: COUNT (anchors and windows per segment, ident bytes
//                      only) and EMIT (one 16-byte store per window; reads the table word as well, for cov).  a = ballot(FMAT),
//                      d = ballot(ident & (UNDS | FDEL)).  A window ends at lane l when l is an anchor or the segment's end; its anchor is
//                      the highest bit of a below l — then it is dirty when d has a bit in [anchor, l) — or the carried anchor with the
//                      carried OR of dirty bits since.  A window may span any number of steps.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <utility>
#include <vector>

#include "common.h"
#include "cns_plan.h"
#include "cns_ranges.h"
#include "scan.h"

static double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static_assert(sizeof(mhip_cns_segment) == 32 && sizeof(mhip_cns_window) == 16, "plan records");

namespace {

__global__ __launch_bounds__(256) void cns_plan_segments(const uint32_t* __restrict__ table, const long long* __restrict__ tb, const int32_t* __restrict__ er,
                                                         const long long* __restrict__ rb, const long long* __restrict__ slot, int nt, int t_index0, int min_cov,
                                                         int min_run, mhip_cns_segment* __restrict__ slots, int32_t* __restrict__ cnt, long long* __restrict__ bad) {
    const int lane = lane_id();
    const unsigned long long lt = (1ull << lane) - 1ull;                // the lanes below this one
    for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < nt; t += (long long)gridDim.x * 4) {
        const uint32_t* __restrict__ tab = table + tb[t];
        const int L = (int)(tb[t + 1] - tb[t]);
        const long long s0 = slot[t];
        const int cap = (int)(slot[t + 1] - s0);
        int n = 0;                              // segments of this template so far
        for (long long r = rb[t]; r < rb[t + 1]; ++r) {
            const int Lr = max(er[2 * r], 0), Rr = min(er[2 * r + 1], L);
            if (Lr >= Rr) continue;
            bool open = false;                  // a run reaches the end of the previous step ...
            int start = 0;                      // ... and began here
            uint32_t nx = 0;
            if (Lr + lane < Rr) nx = tab[Lr + lane];
            for (int p0 = Lr; p0 <= Rr; p0 += 64) {
                const int p = p0 + lane;
                const uint32_t x = nx;
                if (p + 64 < Rr) nx = tab[p + 64];              // the next step's words, in flight under this step
                const bool c = p < Rr && (int)((x >> 8) & 255u) + (int)((x >> 16) & 255u) >= min_cov;
                const unsigned long long m = __ballot(c);
                const bool prev = lane ? ((m >> (lane - 1)) & 1ull) != 0 : open;
                const unsigned long long zb = ~m & lt;
                const int beg = zb ? p0 + 64 - __clzll((long long)zb) : (open ? start : p0);
                const bool acc = !c && prev && p <= Rr && p - beg >= min_run;
                const unsigned long long am = __ballot(acc);
                if (acc) {
                    const int k = n + __popcll(am & lt);
                    if (k < cap) {
                        mhip_cns_segment sg;
                        sg.template_index = t_index0 + (int)t; sg.beg = beg; sg.end = p; sg.n_anchors = 0; sg.win_begin = 0; sg.win_end = 0;
                        slots[s0 + k] = sg;
                    }
                }
                n += __popcll(am);
                if (m >> 63) {
                    const unsigned long long z = ~m;
                    start = z ? p0 + 64 - __clzll((long long)z) : (open ? start : p0);
                    open = true;
                } else open = false;
            }
        }
        if (lane == 0) {
            cnt[t] = min(n, cap);               // (what compact may copy)
            if (n > cap) *bad = 1;              // more runs than the bound allows: the host refuses the plan
        }
    }
}

// out[i] = base + cnt[0] + .. + cnt[i - 1] for i <= n; n = *n_dev - n_base when n_dev is given (a count that only the device knows yet).
// One block of 1024.
__global__ __launch_bounds__(1024) void cns_plan_scan(const int32_t* __restrict__ cnt, long long n, const long long* __restrict__ n_dev, long long n_base,
                                                      long long base, long long* __restrict__ out, long long* __restrict__ total) {
    if (n_dev) n = *n_dev - n_base;
    const long long run = scan_array_1024<long long>(n, base, [&](long long i) { return cnt[i]; }, [&](long long i, long long p) { out[i] = p; });
    if (threadIdx.x == 0) {
        out[n] = run;
        if (total) *total = run;
    }
}

__global__ __launch_bounds__(256) void cns_plan_compact(const mhip_cns_segment* __restrict__ slots, const long long* __restrict__ slot, const long long* __restrict__ segb,
                                                        long long seg_base, int nt, mhip_cns_segment* __restrict__ seg) {
    const int lane = lane_id();
    for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < nt; t += (long long)gridDim.x * 4) {
        const long long o = segb[t] - seg_base, n = segb[t + 1] - segb[t], s0 = slot[t];
        for (long long i = lane; i < n; i += 64) seg[o + i] = slots[s0 + i];
    }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void cns_plan_windows(const uint32_t* __restrict__ table, const uint8_t* __restrict__ ident, const long long* __restrict__ tb,
                                                        int t_index0, mhip_cns_segment* __restrict__ seg, const long long* __restrict__ n_dev, long long seg_base,
                                                        int32_t* __restrict__ wcnt, const long long* __restrict__ wb, long long win_base, mhip_cns_window* __restrict__ win,
                                                        long long* __restrict__ bad) {
    const int lane = lane_id();
    const unsigned long long lt = (1ull << lane) - 1ull;
    const long long nseg = *n_dev - seg_base;
    for (long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += (long long)gridDim.x * 4) {
        const int tl = seg[s].template_index - t_index0, beg = seg[s].beg, end = seg[s].end;
        const uint8_t* __restrict__ id = ident + tb[tl];
        const uint32_t* __restrict__ tab = table + tb[tl];
        const long long w0 = EMIT ? wb[s] - win_base : 0, w1 = EMIT ? wb[s + 1] - win_base : 0;
        bool has = false, dirty = false;        // an anchor has been seen; UNDS / FDEL at or behind the last one
        int start = 0, scov = 0;                // the last anchor and its mat_cnt + ins_cnt
        int nanch = 0;
        long long nw = 0;
        for (int p0 = beg; p0 <= end; p0 += 64) {
            const int p = p0 + lane;
            uint32_t f = 0;
            int cov = 0;
            if (p < end) {
                f = id[p];
                if (EMIT) {
                    const uint32_t x = tab[p];
                    cov = (int)((x >> 8) & 255u) + (int)((x >> 16) & 255u);
                }
            }
            const unsigned long long a = __ballot((f & 1u) != 0);              // FMAT
            const unsigned long long d = __ballot((f & 10u) != 0);             // UNDS | FDEL
            const unsigned long long ab = a & lt;
            const int sl = ab ? 63 - __clzll((long long)ab) : 0;               // the anchor this lane's window began at, if it lies in the step
            const bool here = ab != 0;
            const bool ender = ((a >> lane) & 1ull) != 0 || p == end;
            const bool drt = here ? (d & lt & ~((1ull << sl) - 1ull)) != 0 : (dirty || (d & lt) != 0);
            const bool need = ender && (here || has) && drt;
            const unsigned long long wm = __ballot(need);
            if (EMIT) {
                const int cv = __shfl(cov, sl);
                const long long k = w0 + nw + __popcll(wm & lt);
                if (need && k < w1) {
                    int4 rec;
                    rec.x = here ? p0 + sl : start; rec.y = p; rec.z = here ? cv : scov; rec.w = (int)(seg_base + s);
                    *reinterpret_cast<int4*>(win + k) = rec;
                }
            }
            nw += __popcll(wm);
            nanch += __popcll(a);
            if (a) {
                const int hl = 63 - __clzll((long long)a);
                has = true;
                start = p0 + hl;
                dirty = (d >> hl) != 0;
                if (EMIT) scov = __shfl(cov, hl);
            } else if (has) dirty = dirty || d != 0;
        }
        if (lane == 0) {
            if (EMIT) {
                seg[s].win_begin = wb[s]; seg[s].win_end = wb[s + 1];
                if (w0 + nw != w1) *bad = 1;    // not the windows that were counted: the host refuses the plan
            }
            else { wcnt[s] = (int32_t)nw; seg[s].n_anchors = nanch; }
        }
    }
}

}  // namespace

int cns_plan_launch(mhip_ctx* c, int set, const uint32_t* d_table, const uint8_t* d_ident, int nt, int t_index0, const long long* tb, const int32_t* er,
                    const long long* rb, int min_cov, int min_run, long long seg_base, long long win_base, int64_t* seg_begin, CnsPlanDev* out) {
    *out = CnsPlanDev();
    if (nt <= 0) return 0;
    if (min_run < 1 || min_cov < 1) { mhip_set_error("cns plan: min_cov %d, shortest segment %d", min_cov, min_run); return -1; }
    const long long nr = rb[nt];
    std::vector<long long> head(3 * ((size_t)nt + 1));      // tb, rb, slot: one upload
    long long* slot = head.data() + 2 * ((size_t)nt + 1);
    slot[0] = 0;
    for (int k = 0; k < nt; ++k) {
        const long long L = tb[k + 1] - tb[k];
        long long cap = 0;
        for (long long r = rb[k]; r < rb[k + 1]; ++r) {
            const long long lo = std::max<long long>(er[2 * r], 0), hi = std::min<long long>(er[2 * r + 1], L);
            if (lo < hi) cap += (hi - lo) / min_run + 1;
        }
        slot[k + 1] = slot[k] + cap;
    }
    const long long S = slot[nt];
    if (S == 0) {                               // no range holds a position: no segment, no window
        for (int k = 0; k <= nt; ++k) seg_begin[k] = seg_base;
        return 0;
    }
    if (seg_base + S > 0x7fffffffLL) { mhip_set_error("cns plan: too many segments in one batch"); return -1; }
    memcpy(head.data(), tb, sizeof(long long) * ((size_t)nt + 1));
    memcpy(head.data() + (size_t)nt + 1, rb, sizeof(long long) * ((size_t)nt + 1));
    auto buf = [&](const char* name, size_t bytes, void** p) { return scratch_set(c, name, set, std::max<size_t>(bytes, 16), p); };
    long long *d_head, *d_segb, *d_wb, *d_tot;
    int32_t *d_er, *d_cnt, *d_wcnt;
    mhip_cns_segment *d_slots, *d_seg;
    mhip_cns_window* d_win;
    if (buf("cp_head", sizeof(long long) * head.size(), (void**)&d_head)) return -1;
    if (buf("cp_er", sizeof(int32_t) * 2 * (size_t)nr, (void**)&d_er)) return -1;
    if (buf("cp_slots", sizeof(mhip_cns_segment) * (size_t)S, (void**)&d_slots)) return -1;
    if (buf("cp_cnt", sizeof(int32_t) * (size_t)nt, (void**)&d_cnt)) return -1;
    if (buf("cp_segb", sizeof(long long) * ((size_t)nt + 1), (void**)&d_segb)) return -1;
    if (buf("cp_seg", sizeof(mhip_cns_segment) * (size_t)S, (void**)&d_seg)) return -1;
    if (buf("cp_wcnt", sizeof(int32_t) * (size_t)S, (void**)&d_wcnt)) return -1;
    if (buf("cp_wb", sizeof(long long) * ((size_t)S + 1), (void**)&d_wb)) return -1;
    if (buf("cp_tot", 3 * sizeof(long long), (void**)&d_tot)) return -1;      // windows so far; segments beyond their slots; windows beyond their count
    const long long *d_tb = d_head, *d_rb = d_head + (size_t)nt + 1, *d_slot = d_head + 2 * ((size_t)nt + 1);
    HIPCHK(hipMemcpyAsync(d_head, head.data(), sizeof(long long) * head.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_er, er, sizeof(int32_t) * 2 * (size_t)nr, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_tot, 0, 3 * sizeof(long long), c->stream));
    const unsigned max_grid = (unsigned)c->num_cus * 8;          // 32 waves per CU, grid-stride beyond
    const unsigned grid_t = (unsigned)std::min<long long>(((long long)nt + 3) / 4, max_grid), grid_s = (unsigned)std::min<long long>((S + 3) / 4, max_grid);
    LAUNCH(c, "cns_plan_segments", cns_plan_segments, grid_t, 256, 0, d_table, d_tb, d_er, d_rb, d_slot, nt, t_index0, min_cov, min_run, d_slots, d_cnt, d_tot + 1);
    LAUNCH(c, "cns_plan_scan", cns_plan_scan, 1, 1024, 0, d_cnt, (long long)nt, (const long long*)nullptr, 0LL, seg_base, d_segb, (long long*)nullptr);
    LAUNCH(c, "cns_plan_compact", cns_plan_compact, grid_t, 256, 0, d_slots, d_slot, d_segb, seg_base, nt, d_seg);
    LAUNCH(c, "cns_plan_count", cns_plan_windows<false>, grid_s, 256, 0, d_table, d_ident, d_tb, t_index0, d_seg, d_segb + nt, seg_base, d_wcnt, (const long long*)nullptr,
           win_base, (mhip_cns_window*)nullptr, (long long*)nullptr);
    LAUNCH(c, "cns_plan_scan", cns_plan_scan, 1, 1024, 0, d_wcnt, 0LL, d_segb + nt, seg_base, win_base, d_wb, d_tot);
    HIPCHK(hipGetLastError());
    long long tot[2] = {0, 0};
    const double t_wait = wall_now();
    HIPCHK(hipMemcpyAsync(seg_begin, d_segb, sizeof(long long) * ((size_t)nt + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(tot, d_tot, 2 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));      // the one wait: the windows' buffer is sized by their number (`head` and `tot` live until here)
    out->wait_s = wall_now() - t_wait;
    const long long nseg = seg_begin[nt] - seg_base, nwin = tot[0] - win_base;
    if (tot[1]) { mhip_set_error("cns plan: a template has more segments than its slots hold"); return -1; }
    if (nseg < 0 || nseg > S || nwin < 0) { mhip_set_error("cns plan: inconsistent counts (%lld segments in %lld slots, %lld windows)", nseg, S, nwin); return -1; }
    if (buf("cp_win", sizeof(mhip_cns_window) * (size_t)nwin, (void**)&d_win)) return -1;
    if (nseg > 0) {
        const unsigned grid_e = (unsigned)std::min<long long>((nseg + 3) / 4, max_grid);
        LAUNCH(c, "cns_plan_emit", cns_plan_windows<true>, grid_e, 256, 0, d_table, d_ident, d_tb, t_index0, d_seg, d_segb + nt, seg_base, (int32_t*)nullptr, d_wb, win_base, d_win, d_tot + 2);
        HIPCHK(hipGetLastError());
    }
    out->d_seg = d_seg; out->d_win = d_win; out->d_segb = d_segb; out->d_bad = d_tot + 2; out->nseg = nseg; out->nwin = nwin;
    return 0;
}

extern "C" {

// TEST HOOK (tests/test_gpu_scan.py): cns_plan_scan — scan.h's routine with a base — on a host array, n from the host.
int mhip_debug_scan(mhip_ctx* c, const int32_t* cnt, int64_t n, int64_t base, int64_t* out) {
    HIPCHK(hipSetDevice(c->device));
    if (n < 0 || !out || (n > 0 && !cnt)) { mhip_set_error("debug scan: n %lld, or a NULL array", (long long)n); return -1; }
    int32_t* d_cnt;
    long long* d_out;
    if (c->scratch("ds_cnt", std::max<size_t>(sizeof(int32_t) * (size_t)n, 16), (void**)&d_cnt)) return -1;
    if (c->scratch("ds_out", sizeof(long long) * ((size_t)n + 1), (void**)&d_out)) return -1;
    if (n) HIPCHK(hipMemcpyAsync(d_cnt, cnt, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "cns_plan_scan", cns_plan_scan, 1, 1024, 0, d_cnt, (long long)n, (const long long*)nullptr, 0LL, (long long)base, d_out, (long long*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(long long) * ((size_t)n + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// TEST HOOK (tests/test_gpu_cns_plan.py): cns_effective_ranges and the kernels above on host-supplied tables.  Template k owns
// table / ident [table_begin[k], table_begin[k + 1]) and the mapping ranges (soff, send) ranges[2 * range_begin[k] .. 2 * range_begin[k + 1]).
// The ident bytes are taken as given.  Outputs as mhip_cns_accept_templates_plan's, released with mhip_cns_free.
int mhip_debug_cns_plan(mhip_ctx* c, const mhip_cns_table_item* table, const uint8_t* ident, const int64_t* table_begin, int n_tmpl, const int32_t* ranges,
                        const int64_t* range_begin, int tech, int min_cov, int min_size, mhip_cns_segment** out_segments, int64_t** out_seg_begin,
                        mhip_cns_window** out_windows, int64_t* out_n_windows, int32_t** out_eranges, int64_t** out_erange_begin) {
    HIPCHK(hipSetDevice(c->device));
    if (!out_segments || !out_seg_begin || !out_windows || !out_n_windows || !out_eranges || !out_erange_begin) { mhip_set_error("cns plan: an output pointer is NULL"); return -1; }
    *out_segments = nullptr; *out_seg_begin = nullptr; *out_windows = nullptr; *out_n_windows = 0; *out_eranges = nullptr; *out_erange_begin = nullptr;
    if (min_size < 2 || min_cov < 1) { mhip_set_error("cns plan: min_size %d (>= 2), min_cov %d (>= 1)", min_size, min_cov); return -1; }
    if (n_tmpl < 0 || (n_tmpl > 0 && (table_begin[0] != 0 || range_begin[0] != 0))) { mhip_set_error("cns plan: table_begin / range_begin must start at 0"); return -1; }
    std::vector<long long> tb((size_t)n_tmpl + 1, 0), rb((size_t)n_tmpl + 1, 0);
    std::vector<int32_t> er;
    std::vector<std::pair<int32_t, int32_t>> mr;
    for (int k = 0; k < n_tmpl; ++k) {
        const int64_t L = table_begin[k + 1] - table_begin[k], nm = range_begin[k + 1] - range_begin[k];
        if (L < 0 || L > (1 << 30) || nm < 0) { mhip_set_error("cns plan: template %d has %lld positions, %lld mapping ranges", k, (long long)L, (long long)nm); return -1; }
        mr.clear();
        for (int64_t r = range_begin[k]; r < range_begin[k + 1]; ++r) {
            if (ranges[2 * r] < 0 || ranges[2 * r] > ranges[2 * r + 1] || ranges[2 * r + 1] > L) { mhip_set_error("cns plan: a mapping range of template %d leaves it", k); return -1; }
            mr.emplace_back(ranges[2 * r], ranges[2 * r + 1]);
        }
        cns_effective_ranges(mr, (int)L, tech, min_size, er);
        tb[(size_t)k + 1] = table_begin[k + 1];
        rb[(size_t)k + 1] = (long long)(er.size() / 2);
    }
    const long long W = n_tmpl ? tb[(size_t)n_tmpl] : 0;
    struct Out {
        void *seg = nullptr, *win = nullptr, *er = nullptr, *segb = nullptr, *erb = nullptr;
        ~Out() { free(seg); free(win); free(er); free(segb); free(erb); }
    } o;
    o.segb = calloc((size_t)n_tmpl + 1, sizeof(int64_t));
    o.erb = malloc(sizeof(int64_t) * ((size_t)n_tmpl + 1));
    o.er = malloc(std::max<size_t>(sizeof(int32_t) * er.size(), 1));
    if (!o.segb || !o.erb || !o.er) { mhip_set_error("out of memory"); return -1; }
    for (int k = 0; k <= n_tmpl; ++k) ((int64_t*)o.erb)[k] = rb[(size_t)k];
    if (!er.empty()) memcpy(o.er, er.data(), sizeof(int32_t) * er.size());
    CnsPlanDev pd;
    if (W > 0) {
        uint32_t* d_tab;
        uint8_t* d_id;
        if (c->scratch("cpd_tab", sizeof(uint32_t) * (size_t)W, (void**)&d_tab)) return -1;
        if (c->scratch("cpd_id", (size_t)W, (void**)&d_id)) return -1;
        HIPCHK(hipMemcpyAsync(d_tab, table, sizeof(uint32_t) * (size_t)W, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_id, ident, (size_t)W, hipMemcpyHostToDevice, c->stream));
        if (cns_plan_launch(c, 0, d_tab, d_id, n_tmpl, 0, tb.data(), er.data(), rb.data(), min_cov, cns_plan_min_run(min_size), 0, 0, (int64_t*)o.segb, &pd)) return -1;
    }
    o.seg = malloc(std::max<size_t>(sizeof(mhip_cns_segment) * (size_t)pd.nseg, 1));
    o.win = malloc(std::max<size_t>(sizeof(mhip_cns_window) * (size_t)pd.nwin, 1));
    if (!o.seg || !o.win) { mhip_set_error("out of memory"); return -1; }
    if (pd.nseg) HIPCHK(hipMemcpyAsync(o.seg, pd.d_seg, sizeof(mhip_cns_segment) * (size_t)pd.nseg, hipMemcpyDeviceToHost, c->stream));
    if (pd.nwin) HIPCHK(hipMemcpyAsync(o.win, pd.d_win, sizeof(mhip_cns_window) * (size_t)pd.nwin, hipMemcpyDeviceToHost, c->stream));
    long long bad = 0;
    if (pd.d_bad) HIPCHK(hipMemcpyAsync(&bad, pd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad) { mhip_set_error("cns plan: the windows written are not the windows counted"); return -1; }
    *out_segments = (mhip_cns_segment*)o.seg; *out_seg_begin = (int64_t*)o.segb; *out_windows = (mhip_cns_window*)o.win; *out_n_windows = pd.nwin;
    *out_eranges = (int32_t*)o.er; *out_erange_begin = (int64_t*)o.erb;
    o.seg = o.win = o.er = o.segb = o.erb = nullptr;
    return 0;
}

}  // extern "C"
