// cns_reads.hip — the corrected reads on the device: the rest of consensus_worker (mecat2cns/mecat_correction.cpp:203-239) behind a
// slice's POA (cns_poa.hip), while its table, ident bytes, plan and consensus strings are still in device memory.
//
//   a segment's target   meap_consensus_one_segment, :88-107: every FMAT position i of the segment, ascending, gives table[i].base and,
//                        when the window with sb == i is listed and its `cns` has more than two letters, cns[1 .. len - 1).
//   records              :233 (a target shorter than min_size gives nothing) and output_cns_result, :155-188 (cns_reads.h).
//
//   cns_reads_size     one WAVE per segment: n_anchors + the sum over its windows of max(0, len - 2), lanes over the windows; the size
//                      filter and the number of records (cns_reads_blocks) from that length alone.
//   cns_reads_scan     one block: the kept lengths and the record counts summed (scan.h) — where a segment's letters and records go —
//                      and the two totals the host sizes the output by (the one wait).
//   cns_reads_records  one lane per segment: its <= a few records (cns_reads_block), and per template its first record.
//   cns_reads_letters  one WAVE per kept segment, 64 positions per step as in cns_plan_windows: a = ballot(FMAT).  The windows that begin
//                      in the step are the next popcount-many of the segment's list (they are ascending and each begins on an anchor):
//                      lane l takes window cursor + l, the inner lengths are summed across the lanes (inclusive scan), and the wave
//                      carries the window cursor and the output offset from step to step.  An anchor's letter goes to
//                      offset + (anchors below it in the step) + (inner letters of the windows that begin below it): the lane on the
//                      anchor finds the number of such windows by a binary search over the window lanes.  The inner letters of a window
//                      of at most CNS_READS_SHORT letters are copied by the lane that holds the window (the usual case: a handful of
//                      letters, 64 windows at once); a longer string is copied by the whole wave, 64 consecutive letters per pass, so
//                      that a string of 1 500 letters does not leave 63 lanes idle and its stores land as runs.
// No atomic decides a place: every position is a prefix sum, so the bytes are the same on every run.  Every index that comes from the
// data — window ordinal, cns_begin, output offset — is checked before it is used; a failed check sets the flag word (the convention of
// cns_pieces.hip's d_bad), as does a segment whose letters written are not the letters counted, and the host refuses the result.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <utility>
#include <vector>

#include "common.h"
#include "cns_pieces.h"
#include "cns_plan.h"
#include "cns_poa_dev.h"
#include "cns_ranges.h"
#include "cns_reads.h"
#include "cns_table.h"
#include "scan.h"

static_assert(sizeof(mhip_cns_read) == 32, "read records");

#define CNS_READS_SHORT 8

namespace {

double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

__global__ __launch_bounds__(256) void cns_reads_size(const mhip_cns_segment* __restrict__ seg, long long nseg, long long win_base, long long nwin, const long long* __restrict__ cb,
                                                      long long cns_cap, int min_size, long long* __restrict__ tlen, long long* __restrict__ keep, long long* __restrict__ nrec,
                                                      long long* __restrict__ bad) {
    const int lane = lane_id();
    for (long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += (long long)gridDim.x * 4) {
        const long long w0 = seg[s].win_begin - win_base, w1 = seg[s].win_end - win_base;
        const int na = seg[s].n_anchors;
        bool ok = w0 >= 0 && w0 <= w1 && w1 <= nwin && na >= 0 && (w0 == w1 || cb != nullptr);
        long long sum = 0;
        if (ok)
            for (long long w = w0 + lane; w < w1; w += 64) {
                const long long b0 = cb[w], b1 = cb[w + 1];
                if (b0 < 0 || b1 < b0 || b1 > cns_cap) { ok = false; break; }
                sum += max(0LL, b1 - b0 - 2);
            }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        ok = __ballot(!ok) == 0;
        if (lane == 0) {
            const long long len = ok ? (long long)na + sum : 0;
            const bool kept = len >= (long long)min_size;
            if (!ok) *bad = 1;
            tlen[s] = len; keep[s] = kept ? len : 0; nrec[s] = kept ? cns_reads_blocks(len) : 0;
        }
    }
}

// keep[] and nrec[] (n + 1 entries each) -> their exclusive sums in place; tot[0] = letters kept, tot[1] = records.  One block of 1024.
__global__ __launch_bounds__(1024) void cns_reads_scan(long long* keep, long long* nrec, long long n, long long* __restrict__ tot) {
    const long long bytes = scan_array_1024<long long>(n, 0, [&](long long i) { return keep[i]; }, [&](long long i, long long p) { keep[i] = p; });
    const long long recs = scan_array_1024<long long>(n, 0, [&](long long i) { return nrec[i]; }, [&](long long i, long long p) { nrec[i] = p; });
    if (threadIdx.x == 0) { keep[n] = bytes; nrec[n] = recs; tot[0] = bytes; tot[1] = recs; }
}

// the records of every kept segment, and (the lanes behind the segments') every template's first record
__global__ __launch_bounds__(256) void cns_reads_records(const mhip_cns_segment* __restrict__ seg, long long nseg, const long long* __restrict__ segb, long long seg_base,
                                                         int nt, int t_index0, const int32_t* __restrict__ read_id, const long long* __restrict__ tlen,
                                                         const long long* __restrict__ sbeg, const long long* __restrict__ rbeg, long long nreads, long long seq_bytes,
                                                         mhip_cns_read* __restrict__ reads, long long* __restrict__ tbegin, long long* __restrict__ bad) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nseg + nt + 1; i += (long long)gridDim.x * 256) {
        if (i >= nseg) {
            const long long k = i - nseg, s = segb[k] - seg_base;
            if (s < 0 || s > nseg) { *bad = 1; tbegin[k] = 0; }
            else tbegin[k] = rbeg[s];
            continue;
        }
        const long long r0 = rbeg[i], n = rbeg[i + 1] - r0;
        if (n <= 0) continue;
        const mhip_cns_segment sg = seg[i];
        const int tl = sg.template_index - t_index0;
        const long long len = tlen[i], o = sbeg[i];
        if (tl < 0 || tl >= nt || r0 < 0 || r0 + n > nreads || n != cns_reads_blocks(len) || o < 0 || o + len > seq_bytes || len > 0x7fffffffLL) { *bad = 1; continue; }
        for (long long k = 0; k < n; ++k) {
            long long L, R, rb, re;
            cns_reads_block(len, k, sg.beg, sg.end, &L, &R, &rb, &re);
            mhip_cns_read rec;
            rec.read_id = read_id[tl]; rec.range_beg = (int32_t)rb; rec.range_end = (int32_t)re; rec.size = (int32_t)(R - L); rec.seq_begin = o + L;
            rec.template_index = sg.template_index; rec.segment = (int32_t)(seg_base + i);
            reads[r0 + k] = rec;
        }
    }
}

__global__ __launch_bounds__(256) void cns_reads_letters(const uint32_t* __restrict__ table, const uint8_t* __restrict__ ident, const long long* __restrict__ tb, int nt,
                                                         int t_index0, const mhip_cns_segment* __restrict__ seg, long long nseg, long long seg_base, long long win_base,
                                                         const mhip_cns_window* __restrict__ win, long long nwin, const char* __restrict__ cns, const long long* __restrict__ cb,
                                                         long long cns_cap, const long long* __restrict__ tlen, const long long* __restrict__ sbeg, long long seq_bytes,
                                                         char* __restrict__ seq, long long* __restrict__ bad) {
    const int lane = lane_id();
    const unsigned long long lt = (1ull << lane) - 1ull;                // the lanes below this one
    for (long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += (long long)gridDim.x * 4) {
        const long long lo = sbeg[s], len = sbeg[s + 1] - lo;
        if (len <= 0) continue;                                          // not kept
        const mhip_cns_segment sg = seg[s];
        const int tl = sg.template_index - t_index0;
        const long long hi = lo + len, w0 = sg.win_begin - win_base, w1 = sg.win_end - win_base;
        bool ok = tl >= 0 && tl < nt && lo >= 0 && hi <= seq_bytes && len == tlen[s] && w0 >= 0 && w0 <= w1 && w1 <= nwin && sg.beg >= 0 && sg.beg < sg.end;
        if (ok) ok = (long long)sg.end <= tb[tl + 1] - tb[tl];
        if (!ok) { if (lane == 0) *bad = 1; continue; }
        const uint8_t* __restrict__ id = ident + tb[tl];
        const uint32_t* __restrict__ tab = table + tb[tl];
        long long off = lo, wc = w0;            // carried from step to step: where the step's first letter goes, the next window of the list
        bool fail = false;
        for (int p0 = sg.beg; p0 < sg.end; p0 += 64) {
            const int p = p0 + lane;
            const bool anchor = p < sg.end && (id[p] & 1u) != 0;       // FMAT
            const unsigned long long a = __ballot(anchor);
            if (a == 0) continue;
            // the windows that begin in this step: the next of the list, one per lane
            const long long wi = wc + lane;
            int wpos = 64;                       // the window's first position, counted from p0 (64: no window on this lane)
            long long il = 0, src = 0;
            if (wi < w1) {
                const mhip_cns_window x = win[wi];
                if (x.sb < p0 + 64) {
                    const long long b0 = cb[wi], b1 = cb[wi + 1];
                    wpos = x.sb - p0;
                    if (wpos < 0 || ((a >> wpos) & 1ull) == 0 || (long long)x.segment != seg_base + s || b0 < 0 || b1 < b0 || b1 > cns_cap) { fail = true; wpos = 0; }
                    else { il = max(0LL, b1 - b0 - 2); src = b0 + 1; }
                }
            }
            const unsigned long long inm = __ballot(wpos < 64);
            const int nin = __popcll(inm);
            if (inm != (nin == 64 ? ~0ull : (1ull << nin) - 1ull)) fail = true;      // (the list is ascending: the step's windows are its next nin)
            long long incl = il;                 // inner letters of the windows on this lane and below
            for (int o = 1; o < 64; o <<= 1) {
                const long long y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            // windows that begin below this lane's position: the first window lane whose wpos is not below `lane`
            int blo = 0, bhi = 64;
            for (int it = 0; it < 7; ++it) {
                const int mid = min((blo + bhi) >> 1, 63);
                const int v = __shfl(wpos, mid);
                if (blo < bhi) { if (v < lane) blo = mid + 1; else bhi = mid; }
            }
            const long long below = __shfl(incl, max(blo - 1, 0));
            if (anchor) {
                const long long d = off + __popcll(a & lt) + (blo > 0 ? below : 0);
                if (d >= lo && d < hi) seq[d] = (char)(tab[p] & 255u);
                else fail = true;
            }
            const long long dst = off + (wpos < 64 ? __popcll(a & ((1ull << wpos) - 1ull)) : 0) + 1 + (incl - il);
            if (il > 0 && (dst < lo || dst + il > hi)) { fail = true; il = 0; }
            if (il > 0 && il <= CNS_READS_SHORT)
                for (long long i = 0; i < il; ++i) seq[dst + i] = cns[src + i];
            unsigned long long lm = __ballot(il > CNS_READS_SHORT);
            while (lm) {                         // a long string: the whole wave, 64 consecutive letters per pass
                const int k = __ffsll((long long)lm) - 1;
                lm &= lm - 1;
                const long long n = __shfl(il, k), sk = __shfl(src, k), dk = __shfl(dst, k);
                for (long long i = lane; i < n; i += 64) seq[dk + i] = cns[sk + i];
            }
            off += __popcll(a) + __shfl(incl, 63);
            wc += nin;
        }
        const bool any = __ballot(fail) != 0;
        if (lane == 0 && (any || off != hi || wc != w1)) *bad = 1;      // not the letters that were counted: the host refuses the result
    }
}

}  // namespace

int cns_reads_launch(mhip_ctx* c, int set, const uint32_t* d_table, const uint8_t* d_ident, int nt, int t_index0, const long long* tb, const int32_t* read_id,
                     const mhip_cns_segment* d_seg, long long nseg, const long long* d_segb, long long seg_base, long long win_base, const mhip_cns_window* d_win, long long nwin,
                     const char* d_cns, const long long* d_cb, long long cns_cap, int min_size, CnsReadsDev* out) {
    *out = CnsReadsDev();
    if (nseg <= 0 || nt <= 0) return 0;
    if (min_size < 2) { mhip_set_error("cns reads: min_size %d (>= 2)", min_size); return -1; }
    if (nwin > 0 && (!d_cb || !d_win)) { mhip_set_error("cns reads: %lld windows without their consensus", nwin); return -1; }
    auto buf = [&](const char* name, size_t bytes, void** p) { return scratch_set(c, name, set, std::max<size_t>(bytes, 16), p); };
    const size_t n1 = (size_t)nseg + 1, t1 = (size_t)nt + 1;
    long long *d_head, *d_tlen, *d_sbeg, *d_rbeg, *d_tot, *d_tbegin;
    int32_t* d_rid;
    if (buf("cr_head", sizeof(long long) * t1, (void**)&d_head)) return -1;
    if (buf("cr_rid", sizeof(int32_t) * t1, (void**)&d_rid)) return -1;
    if (buf("cr_tlen", sizeof(long long) * n1, (void**)&d_tlen)) return -1;
    if (buf("cr_sbeg", sizeof(long long) * n1, (void**)&d_sbeg)) return -1;
    if (buf("cr_rbeg", sizeof(long long) * n1, (void**)&d_rbeg)) return -1;
    if (buf("cr_tbegin", sizeof(long long) * t1, (void**)&d_tbegin)) return -1;
    if (buf("cr_tot", 3 * sizeof(long long), (void**)&d_tot)) return -1;      // letters kept, records, the flag word
    HIPCHK(hipMemcpyAsync(d_head, tb, sizeof(long long) * t1, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_rid, read_id, sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_tot, 0, 3 * sizeof(long long), c->stream));
    long long* d_bad = d_tot + 2;
    const unsigned max_grid = (unsigned)c->num_cus * 8;
    const unsigned grid_s = (unsigned)std::max<long long>(1, std::min<long long>((nseg + 3) / 4, max_grid));
    LAUNCH(c, "cns_reads_size", cns_reads_size, grid_s, 256, 0, d_seg, nseg, win_base, nwin, d_cb, cns_cap, min_size, d_tlen, d_sbeg, d_rbeg, d_bad);
    LAUNCH(c, "cns_reads_scan", cns_reads_scan, 1, 1024, 0, d_sbeg, d_rbeg, nseg, d_tot);
    HIPCHK(hipGetLastError());
    long long tot[3] = {0, 0, 0};
    const double t_wait = wall_now();
    HIPCHK(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));      // the one wait: the two totals size the output (the caller's tb and read_id live until here)
    out->wait_s = wall_now() - t_wait;
    if (tot[2]) { mhip_set_error("cns reads: a segment's windows or their strings leave their arrays"); return -1; }
    if (tot[0] < 0 || tot[1] < 0 || tot[1] > tot[0]) { mhip_set_error("cns reads: inconsistent totals (%lld letters, %lld records)", tot[0], tot[1]); return -1; }
    char* d_seq;
    mhip_cns_read* d_reads;
    if (buf("cr_seq", (size_t)tot[0] + 16, (void**)&d_seq)) return -1;      // (+ 16: cns_text_write reads whole aligned 16-byte words)
    if (buf("cr_reads", sizeof(mhip_cns_read) * (size_t)tot[1], (void**)&d_reads)) return -1;
    const unsigned grid_r = (unsigned)std::max<long long>(1, std::min<long long>((nseg + nt + 1 + 255) / 256, (long long)max_grid * 4));
    LAUNCH(c, "cns_reads_records", cns_reads_records, grid_r, 256, 0, d_seg, nseg, d_segb, seg_base, nt, t_index0, d_rid, d_tlen, d_sbeg, d_rbeg, tot[1], tot[0], d_reads, d_tbegin,
           d_bad);
    if (tot[0] > 0)
        LAUNCH(c, "cns_reads_letters", cns_reads_letters, grid_s, 256, 0, d_table, d_ident, d_head, nt, t_index0, d_seg, nseg, seg_base, win_base, d_win, nwin, d_cns, d_cb, cns_cap,
               d_tlen, d_sbeg, tot[0], d_seq, d_bad);
    HIPCHK(hipGetLastError());
    out->d_reads = d_reads; out->d_seq = d_seq; out->d_tbegin = d_tbegin; out->d_bad = d_bad; out->nreads = tot[1]; out->seq_bytes = tot[0];
    return 0;
}

namespace {

const char* const READS_BAD = "cns reads: an index left its array, or the letters written are not the letters counted";

struct ReadsOut {
    void *reads = nullptr, *rb = nullptr, *seq = nullptr;
    ~ReadsOut() { free(reads); free(rb); free(seq); }
};

// a launch's reads to malloc'ed host arrays (rb may stay NULL: no per-template array wanted); waits for the stream
int download_reads(mhip_ctx* c, const CnsReadsDev& rd, int nt, ReadsOut& o, bool want_rb) {
    o.reads = malloc(std::max<size_t>(sizeof(mhip_cns_read) * (size_t)rd.nreads, 1));
    o.seq = malloc(std::max<size_t>((size_t)rd.seq_bytes, 1));
    if (want_rb) o.rb = calloc((size_t)nt + 1, sizeof(int64_t));
    if (!o.reads || !o.seq || (want_rb && !o.rb)) { mhip_set_error("out of memory"); return -1; }
    long long bad = 0;
    if (rd.nreads) HIPCHK(hipMemcpyAsync(o.reads, rd.d_reads, sizeof(mhip_cns_read) * (size_t)rd.nreads, hipMemcpyDeviceToHost, c->stream));
    if (rd.seq_bytes) HIPCHK(hipMemcpyAsync(o.seq, rd.d_seq, (size_t)rd.seq_bytes, hipMemcpyDeviceToHost, c->stream));
    if (want_rb && rd.d_tbegin) HIPCHK(hipMemcpyAsync(o.rb, rd.d_tbegin, sizeof(int64_t) * ((size_t)nt + 1), hipMemcpyDeviceToHost, c->stream));
    if (rd.d_bad) HIPCHK(hipMemcpyAsync(&bad, rd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad) { mhip_set_error("%s", READS_BAD); return -1; }
    return 0;
}

}  // namespace

extern "C" {

int mhip_cns_format_reads(const mhip_cns_read* reads, int64_t n, const char* seq, int64_t seq_bytes, char** out_text, int64_t* out_bytes) {
    if (!out_text || !out_bytes) { mhip_set_error("cns reads: an output pointer is NULL"); return -1; }
    *out_text = nullptr; *out_bytes = 0;
    if (n < 0 || seq_bytes < 0 || (n > 0 && !reads) || (seq_bytes > 0 && !seq)) { mhip_set_error("cns reads: %lld records, %lld letters, or a NULL array", (long long)n, (long long)seq_bytes); return -1; }
    size_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        const mhip_cns_read& r = reads[i];
        if (r.size < 0 || r.seq_begin < 0 || r.seq_begin + r.size > seq_bytes) { mhip_set_error("cns reads: record %lld leaves the letters", (long long)i); return -1; }
        total += (size_t)snprintf(nullptr, 0, ">%d_%d_%d_%d\n", r.read_id, r.range_beg, r.range_end, r.size) + (size_t)r.size + 1;
    }
    char* text = (char*)malloc(total + 64);      // (snprintf writes a terminator behind the last header it formats)
    if (!text) { mhip_set_error("out of memory"); return -1; }
    size_t p = 0;
    for (int64_t i = 0; i < n; ++i) {
        const mhip_cns_read& r = reads[i];
        p += (size_t)snprintf(text + p, 64, ">%d_%d_%d_%d\n", r.read_id, r.range_beg, r.range_end, r.size);
        memcpy(text + p, seq + r.seq_begin, (size_t)r.size);
        p += (size_t)r.size;
        text[p++] = '\n';
    }
    *out_text = text; *out_bytes = (int64_t)p;
    return 0;
}

// TEST HOOK (tests/test_gpu_cns_reads.py): the kernels above on host-supplied arrays; see mecat_hip.h
int mhip_debug_cns_reads(mhip_ctx* c, const mhip_cns_table_item* table, const uint8_t* ident, const int64_t* table_begin, int n_tmpl, const int32_t* read_id,
                         const mhip_cns_segment* segments, int64_t n_seg, const mhip_cns_window* windows, int64_t n_win, const char* cns, const int64_t* cns_begin, int min_size,
                         mhip_cns_read** out_reads, int64_t** out_read_begin, char** out_seq, int64_t* out_seq_bytes) {
    HIPCHK(hipSetDevice(c->device));
    if (!out_reads || !out_read_begin || !out_seq || !out_seq_bytes) { mhip_set_error("cns reads: an output pointer is NULL"); return -1; }
    *out_reads = nullptr; *out_read_begin = nullptr; *out_seq = nullptr; *out_seq_bytes = 0;
    if (min_size < 2) { mhip_set_error("cns reads: min_size %d (>= 2)", min_size); return -1; }
    if (n_tmpl < 0 || n_seg < 0 || n_win < 0 || n_seg > 0x7fffffffLL || n_win > 0x7fffffffLL) { mhip_set_error("cns reads: %d templates, %lld segments, %lld windows", n_tmpl, (long long)n_seg, (long long)n_win); return -1; }
    if (n_tmpl > 0 && table_begin[0] != 0) { mhip_set_error("cns reads: table_begin must start at 0"); return -1; }
    std::vector<long long> tb((size_t)n_tmpl + 1, 0), segb((size_t)n_tmpl + 1, 0);
    for (int k = 0; k < n_tmpl; ++k) {
        if (table_begin[k + 1] < table_begin[k] || table_begin[k + 1] - table_begin[k] > (1 << 30)) { mhip_set_error("cns reads: template %d has %lld positions", k, (long long)(table_begin[k + 1] - table_begin[k])); return -1; }
        tb[(size_t)k + 1] = table_begin[k + 1];
    }
    if (cns_begin[0] != 0) { mhip_set_error("cns reads: cns_begin must start at 0"); return -1; }
    for (int64_t w = 0; w < n_win; ++w)
        if (cns_begin[w + 1] < cns_begin[w]) { mhip_set_error("cns reads: cns_begin does not ascend at window %lld", (long long)w); return -1; }
    int64_t wnext = 0;
    for (int64_t s = 0; s < n_seg; ++s) {
        const mhip_cns_segment& g = segments[s];
        if (g.template_index < 0 || g.template_index >= n_tmpl || (s && g.template_index < segments[s - 1].template_index)) { mhip_set_error("cns reads: segment %lld is not in template order (template %d)", (long long)s, g.template_index); return -1; }
        if (g.beg < 0 || g.beg >= g.end || g.end > tb[(size_t)g.template_index + 1] - tb[(size_t)g.template_index]) { mhip_set_error("cns reads: segment %lld (%d, %d) lies outside its template", (long long)s, g.beg, g.end); return -1; }
        if (g.win_begin > g.win_end || g.win_begin < wnext || g.win_end > n_win) { mhip_set_error("cns reads: segment %lld owns windows %lld .. %lld: not win_begin <= win_end, ascending and inside the list", (long long)s, (long long)g.win_begin, (long long)g.win_end); return -1; }
        wnext = g.win_end;
        for (int64_t w = g.win_begin; w < g.win_end; ++w) {
            const mhip_cns_window& x = windows[w];
            if (x.sb >= x.se) { mhip_set_error("cns reads: window %lld is not sb < se (%d, %d)", (long long)w, x.sb, x.se); return -1; }
            if (w > g.win_begin && windows[w - 1].se > x.sb) { mhip_set_error("cns reads: windows %lld and %lld are not ascending and disjoint", (long long)w - 1, (long long)w); return -1; }
            if (x.sb < g.beg || x.se > g.end || (int64_t)x.segment != s) { mhip_set_error("cns reads: window %lld (%d, %d) lies outside its segment", (long long)w, x.sb, x.se); return -1; }
        }
        ++segb[(size_t)g.template_index + 1];
    }
    for (int k = 0; k < n_tmpl; ++k) segb[(size_t)k + 1] += segb[(size_t)k];
    ReadsOut o;
    CnsReadsDev rd;
    const long long W = tb[(size_t)n_tmpl], CB = cns_begin[n_win];
    if (n_seg > 0 && W > 0) {
        uint32_t* d_tab; uint8_t* d_id; mhip_cns_segment* d_seg; mhip_cns_window* d_win; long long *d_segb, *d_cb; char* d_cns;
        if (c->scratch("crd_tab", sizeof(uint32_t) * (size_t)W, (void**)&d_tab)) return -1;
        if (c->scratch("crd_id", (size_t)W, (void**)&d_id)) return -1;
        if (c->scratch("crd_seg", sizeof(mhip_cns_segment) * (size_t)n_seg, (void**)&d_seg)) return -1;
        if (c->scratch("crd_win", std::max<size_t>(sizeof(mhip_cns_window) * (size_t)n_win, 16), (void**)&d_win)) return -1;
        if (c->scratch("crd_segb", sizeof(long long) * ((size_t)n_tmpl + 1), (void**)&d_segb)) return -1;
        if (c->scratch("crd_cb", sizeof(long long) * ((size_t)n_win + 1), (void**)&d_cb)) return -1;
        if (c->scratch("crd_cns", std::max<size_t>((size_t)CB, 16), (void**)&d_cns)) return -1;
        HIPCHK(hipMemcpyAsync(d_tab, table, sizeof(uint32_t) * (size_t)W, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_id, ident, (size_t)W, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_seg, segments, sizeof(mhip_cns_segment) * (size_t)n_seg, hipMemcpyHostToDevice, c->stream));
        if (n_win) HIPCHK(hipMemcpyAsync(d_win, windows, sizeof(mhip_cns_window) * (size_t)n_win, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_segb, segb.data(), sizeof(long long) * ((size_t)n_tmpl + 1), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_cb, cns_begin, sizeof(long long) * ((size_t)n_win + 1), hipMemcpyHostToDevice, c->stream));
        if (CB) HIPCHK(hipMemcpyAsync(d_cns, cns, (size_t)CB, hipMemcpyHostToDevice, c->stream));
        if (cns_reads_launch(c, 0, d_tab, d_id, n_tmpl, 0, tb.data(), read_id, d_seg, n_seg, d_segb, 0, 0, d_win, n_win, d_cns, d_cb, CB, min_size, &rd)) return -1;
    }
    if (download_reads(c, rd, n_tmpl, o, true)) return -1;
    *out_reads = (mhip_cns_read*)o.reads; *out_read_begin = (int64_t*)o.rb; *out_seq = (char*)o.seq; *out_seq_bytes = rd.seq_bytes;
    o.reads = o.rb = o.seq = nullptr;
    return 0;
}

// TEST HOOK (tests/test_gpu_cns_reads.py): the whole back end on one template through the accept stage's launchers; see mecat_hip.h
int mhip_debug_cns_correct(mhip_ctx* c, const char* buf, int64_t bytes, const int64_t* off, const int32_t* len, const int32_t* soff, const int32_t* send, int n_pairs,
                           const char* tmpl_letters, int tmpl_len, int tech, int min_cov, int min_size, int read_id, mhip_cns_read** out_reads, int64_t* out_n_reads,
                           char** out_seq, int64_t* out_seq_bytes) {
    HIPCHK(hipSetDevice(c->device));
    if (!out_reads || !out_n_reads || !out_seq || !out_seq_bytes) { mhip_set_error("cns reads: an output pointer is NULL"); return -1; }
    *out_reads = nullptr; *out_n_reads = 0; *out_seq = nullptr; *out_seq_bytes = 0;
    if (min_size < 2 || min_cov < 1) { mhip_set_error("cns reads: min_size %d (>= 2), min_cov %d (>= 1)", min_size, min_cov); return -1; }
    if (n_pairs < 0 || n_pairs > 100) { mhip_set_error("cns reads: %d pairs (at most 100: MAX_CNS_OVLPS)", n_pairs); return -1; }
    if (tmpl_len <= 0 || tmpl_len > (1 << 30)) { mhip_set_error("cns reads: empty template"); return -1; }
    std::vector<CnsTabItem> titems((size_t)n_pairs);
    std::vector<CnsPieceItem> pitems((size_t)n_pairs);
    std::vector<std::pair<int32_t, int32_t>> mr;
    for (int p = 0; p < n_pairs; ++p) {
        if (len[p] < 1) { mhip_set_error("cns reads: pair %d has len %d (< 1)", p, len[p]); return -1; }
        if (off[p] < 0 || off[p] + 2 * ((int64_t)len[p] + 1) > bytes) { mhip_set_error("cns reads: pair %d lies outside the buffer", p); return -1; }
        if (soff[p] < 0 || send[p] < 0) { mhip_set_error("cns reads: pair %d has negative coordinates", p); return -1; }
        const char* q = buf + off[p];
        const char* s = q + len[p] + 1;
        int64_t bases = 0;
        for (int i = 0; i < len[p]; ++i) {
            if (q[i] != '-' && s[i] != '-' && q[i] != s[i]) { mhip_set_error("cns reads: pair %d has a mismatch column (%d)", p, i); return -1; }
            bases += s[i] != '-';
        }
        if ((int64_t)send[p] - soff[p] != bases) { mhip_set_error("cns reads: pair %d: send - soff = %lld, but its template string holds %lld bases", p, (long long)send[p] - soff[p], (long long)bases); return -1; }
        if ((int64_t)soff[p] + bases > tmpl_len) { mhip_set_error("cns reads: pair %d leaves the template", p); return -1; }
        CnsTabItem& ti = titems[(size_t)p];
        ti.off = (unsigned long long)off[p]; ti.tab = 0; ti.aln_size = len[p]; ti.soff = soff[p]; ti.tab_len = tmpl_len; ti.pad = 0;
        CnsPieceItem& pi = pitems[(size_t)p];
        pi.off = (unsigned long long)off[p]; pi.aln_size = len[p]; pi.soff = soff[p]; pi.send = send[p]; pi.tl = 0;
        mr.emplace_back(soff[p], send[p]);
    }
    std::vector<int32_t> er;
    cns_effective_ranges(mr, tmpl_len, tech, min_size, er);
    char *d_buf, *d_let;
    CnsTabItem* d_items;
    uint32_t* d_tab;
    uint8_t* d_id;
    if (c->scratch("crc_buf", (size_t)std::max<int64_t>(bytes, 1) + 128, (void**)&d_buf)) return -1;
    if (c->scratch("crc_items", sizeof(CnsTabItem) * (size_t)std::max(n_pairs, 1), (void**)&d_items)) return -1;
    if (c->scratch("crc_let", (size_t)tmpl_len, (void**)&d_let)) return -1;
    if (c->scratch("crc_tab", sizeof(uint32_t) * (size_t)tmpl_len, (void**)&d_tab)) return -1;
    if (c->scratch("crc_id", (size_t)tmpl_len, (void**)&d_id)) return -1;
    if (bytes > 0) HIPCHK(hipMemcpyAsync(d_buf, buf, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    if (n_pairs > 0) HIPCHK(hipMemcpyAsync(d_items, titems.data(), sizeof(CnsTabItem) * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_let, tmpl_letters, (size_t)tmpl_len, hipMemcpyHostToDevice, c->stream));
    if (cns_table_launch(c, nullptr, d_buf, d_items, n_pairs, d_tab, d_id, tmpl_len, nullptr, nullptr, 0, d_let)) return -1;
    const long long tb[2] = {0, tmpl_len}, rb[2] = {0, (long long)(er.size() / 2)}, afirst[2] = {0, n_pairs};
    int64_t segb[2] = {0, 0};
    CnsPlanDev pd; CnsPiecesDev qd; CnsPoaDev od; CnsReadsDev rd;
    if (cns_plan_launch(c, 0, d_tab, d_id, 1, 0, tb, er.data(), rb, min_cov, cns_plan_min_run(min_size), 0, 0, segb, &pd)) return -1;      // (waits: `titems` lives long enough)
    if (pd.nwin > 0 && n_pairs > 0) {
        if (cns_pieces_launch(c, 0, d_buf, pitems.data(), n_pairs, 0, 1, 0, afirst, tb, pd.d_seg, pd.nseg, pd.d_segb, 0, 0, pd.d_win, pd.nwin, &qd)) return -1;
        if (cns_poa_launch(c, 0, d_buf, qd, n_pairs, 0, pd.d_win, pd.nwin, &od)) return -1;
    }
    const int32_t rid = read_id;
    if (cns_reads_launch(c, 0, d_tab, d_id, 1, 0, tb, &rid, pd.d_seg, pd.nseg, pd.d_segb, 0, 0, pd.d_win, pd.nwin, od.d_cns, od.d_cb, od.cap, min_size, &rd)) return -1;
    long long bad[3] = {0, 0, 0};
    if (pd.d_bad) HIPCHK(hipMemcpyAsync(&bad[0], pd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    if (qd.d_bad) HIPCHK(hipMemcpyAsync(&bad[1], qd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    if (od.d_bad) HIPCHK(hipMemcpyAsync(&bad[2], od.d_bad, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    ReadsOut o;
    if (download_reads(c, rd, 1, o, false)) return -1;
    if (bad[0]) { mhip_set_error("cns plan: the windows written are not the windows counted"); return -1; }
    if (bad[1]) { mhip_set_error("cns pieces: an index left its array, or the pieces written are not the pieces counted"); return -1; }
    if (bad[2]) { mhip_set_error("cns poa: a window's graph left its workspace bound, or a piece leaves its backbone"); return -1; }
    *out_reads = (mhip_cns_read*)o.reads; *out_n_reads = rd.nreads; *out_seq = (char*)o.seq; *out_seq_bytes = rd.seq_bytes;
    o.reads = o.seq = nullptr;
    return 0;
}

}  // extern "C"
