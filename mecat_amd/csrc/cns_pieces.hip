// cns_pieces.hip — what mecat2cns hands to the POA for a listed window, as descriptors, computed while a slice's aligned strings and plan
// are still in device memory.  For a window (sb, se) meap_cns_one_indel (mecat2cns/mecat_correction.cpp:62-78) asks every accepted
// alignment of the template, in add order, for its part of the window: CnsAln::retrieve_aln_subseqs (reads_correction_aux.h:47-68).  A
// CnsAln carries a cursor (aln_idx, soff) that only moves forward; the calls of a template come in plan order, windows ascending and
// disjoint.  Restated without the cursor (tests/cns_pieces_ref.py holds the literal loops and this form against each other):
//     pos(c)   template position of column c: soff0 + the non-gap characters of saln[1 .. c]; pos(0) = soff0 whatever column 0 holds
//     F(p)     the first column with pos(c) == p, or n - 1 if there is none: column 0 for soff0, otherwise a column with a template base
//     a call is true   iff n >= 2, se > soff0, sb < send, and the template's previous listed window (sb', se') does not satisfy
//                      se' > soff0 && sb' < send && F(se') >= n - 1 — that window left the cursor on the last column for good (an earlier
//                      one that did has only false calls behind it, up to and including the previous one, or is the previous one)
//     it returns       columns F(max(soff0, sb)) .. F(se) and sb_out = max(soff0, sb)
//
//   cns_pieces_tmplwin  one LANE per template: its first window, from the plan's seg_begin and the segments' win_begin
//   cns_pieces_mark     one LANE per window: the window's number goes to start[sb] and to end[se - 1] of two position-indexed arrays
//                       (one 32-bit word per template position each, -1 elsewhere).  Windows are disjoint: every word has one writer.
//   cns_pieces_range    one LANE per alignment: the windows [w_lo, w_hi) of its template with se > soff0 and sb < send (two binary
//                       searches in the template's sorted windows), none when n < 2; their number is the alignment's share of the
//                       boundary-column arrays, placed by cns_pieces_scan
//   cns_pieces_cols     one WAVE per alignment, 64 columns of saln per step as in cns_table_tally: a ballot of the template bases, a
//                       popcount prefix for pos(c), the position carried from step to step.  A lane on a first column looks its position
//                       up in the two arrays and stores its column as F(sb) / F(se) of the window found there, in the alignment's share.
//   cns_pieces_walk     one WAVE per window, COUNT and EMIT instantiations of one walk: the template's alignments 64 at a time (two
//                       rounds for 100), validity by the rule above, a piece's place = the window's first piece (cns_pieces_scan over the
//                       counts) + the valid alignments before it (carried) + a popcount prefix of the ballot.  One 16-byte store per piece.
// No atomic decides a place.  Every index that comes from the data — template, window ordinal, column, piece slot — is checked before it
// is used; what fails sets a flag word and the host refuses the result.  The strings are read byte by byte inside [0, n) only.
//
// Buffers: the boundary columns and the pieces are sized by T = sum over the alignments of (w_hi - w_lo) — every overlapping (alignment,
// window) pair, of which only the exhaustion rule drops one, so T is a tight bound on the pieces.  The host WAITS for T once per launch
// (a second wait per slice, behind the plan's); the number of pieces itself is not waited for: the caller copies T slots and reads
// the count from d_pb[nwin] when the copies have landed.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "common.h"
#include "cns_pieces.h"
#include "scan.h"

static_assert(sizeof(mhip_cns_piece) == 16 && sizeof(CnsPieceItem) == 24, "piece records");

namespace {

double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

__global__ __launch_bounds__(256) void cns_pieces_tmplwin(const mhip_cns_segment* __restrict__ seg, long long nseg, const long long* __restrict__ segb, long long seg_base,
                                                          long long win_base, long long nwin, int nt, long long* __restrict__ twb, long long* __restrict__ bad) {
    const long long tl = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tl > nt) return;
    const long long s0 = segb[tl] - seg_base;
    long long v = nwin;                         // (no segment at or behind this template: its windows begin where the windows end)
    if (s0 < 0 || s0 > nseg) *bad = 1;
    else if (s0 < nseg) v = seg[s0].win_begin - win_base;
    if (v < 0 || v > nwin) { *bad = 1; v = nwin; }
    twb[tl] = v;
}

__global__ __launch_bounds__(256) void cns_pieces_mark(const mhip_cns_window* __restrict__ win, long long nwin, const mhip_cns_segment* __restrict__ seg, long long nseg,
                                                       long long seg_base, int t_index0, int nt, const long long* __restrict__ tb, int32_t* __restrict__ startw,
                                                       int32_t* __restrict__ endw, int32_t* __restrict__ wtl, long long* __restrict__ bad) {
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < nwin; w += (long long)gridDim.x * 256) {
        const mhip_cns_window x = win[w];
        const long long s = (long long)x.segment - seg_base;
        int tl = -1;
        if (s >= 0 && s < nseg) {
            tl = seg[s].template_index - t_index0;
            if (tl < 0 || tl >= nt) tl = -1;
        }
        if (tl >= 0) {
            const long long L = tb[tl + 1] - tb[tl];
            if (x.sb >= 0 && x.sb < x.se && x.se <= L) {
                startw[tb[tl] + x.sb] = (int32_t)w;
                endw[tb[tl] + x.se - 1] = (int32_t)w;
            } else tl = -1;
        }
        if (tl < 0) *bad = 1;
        wtl[w] = tl;
    }
}

__global__ __launch_bounds__(256) void cns_pieces_range(const CnsPieceItem* __restrict__ items, long long na, int nt, const long long* __restrict__ twb,
                                                        const mhip_cns_window* __restrict__ win, long long nwin, int2* __restrict__ rng, int32_t* __restrict__ cnt,
                                                        long long* __restrict__ bad) {
    for (long long a = (long long)blockIdx.x * 256 + threadIdx.x; a < na; a += (long long)gridDim.x * 256) {
        const CnsPieceItem it = items[a];
        long long lo = 0, hi = 0;
        if (it.tl < 0 || it.tl >= nt) *bad = 1;
        else {
            const long long w0 = twb[it.tl], w1 = twb[it.tl + 1];
            if (w0 < 0 || w0 > w1 || w1 > nwin) *bad = 1;
            else if (it.aln_size < 2) lo = hi = w0;          // aln_idx >= aln_size - 1 from the start: every call is false
            else {
                long long l = w0, h = w1;                     // the first window with se > soff0
                while (l < h) {
                    const long long m = (l + h) >> 1;
                    if (win[m].se > it.soff) h = m; else l = m + 1;
                }
                lo = l;
                h = w1;                                       // the first window with sb >= send (at or behind lo)
                while (l < h) {
                    const long long m = (l + h) >> 1;
                    if (win[m].sb >= it.send) h = m; else l = m + 1;
                }
                hi = l;
            }
        }
        rng[a] = make_int2((int)lo, (int)hi);
        cnt[a] = (int32_t)(hi - lo);
    }
}

// out[i] = cnt[0] + .. + cnt[i - 1] for i <= n, in 64 bits; *total = out[n].  One block of 1024.
__global__ __launch_bounds__(1024) void cns_pieces_scan(const int32_t* __restrict__ cnt, long long n, long long* __restrict__ out, long long* __restrict__ total) {
    const long long run = scan_array_1024<long long>(n, 0, [&](long long i) { return cnt[i]; }, [&](long long i, long long p) { out[i] = p; });
    if (threadIdx.x == 0) {
        out[n] = run;
        if (total) *total = run;
    }
}

__global__ __launch_bounds__(256) void cns_pieces_cols(const char* __restrict__ str, const CnsPieceItem* __restrict__ items, long long na, const int2* __restrict__ rng,
                                                       const long long* __restrict__ abase, long long T, const long long* __restrict__ tb, int nt,
                                                       const mhip_cns_window* __restrict__ win, const int32_t* __restrict__ startw, const int32_t* __restrict__ endw,
                                                       int32_t* __restrict__ cols, int32_t* __restrict__ cole, long long* __restrict__ bad) {
    const int lane = lane_id();
    const unsigned long long le = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);      // this lane and the lanes below it
    for (long long a = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); a < na; a += (long long)gridDim.x * 4) {
        const CnsPieceItem it = items[a];
        const int2 rg = rng[a];
        const int nw = rg.y - rg.x;
        if (nw <= 0) continue;
        const long long base = abase[a];
        if (base < 0 || base + nw > T || it.tl < 0 || it.tl >= nt) {
            if (lane == 0) *bad = 1;
            continue;
        }
        const long long tb0 = tb[it.tl];
        const int L = (int)(tb[it.tl + 1] - tb0);
        const int n = it.aln_size;
        const char* __restrict__ s = str + it.off + n + 1;
        const int last_se = win[rg.y - 1].se;   // no boundary of the alignment's windows lies behind it
        int pos = it.soff;                      // pos() of the column in front of the step
        char ns = 0;
        if (lane < n) ns = s[lane];
        for (int c0 = 0; c0 < n && pos <= last_se; c0 += 64) {
            const int c = c0 + lane;
            const bool valid = c < n;
            const char cs = ns;
            if (c + 64 < n) ns = s[c + 64];     // the next step's characters, in flight under this step
            const unsigned long long ng = __ballot(valid && cs != '-' && c > 0);      // columns that move the position
            const int p = pos + __popcll(ng & le);
            if (valid && (c == 0 || cs != '-')) {      // the first column at position p
                if (p >= 0 && p < L) {
                    const int w = startw[tb0 + p];
                    if (w >= rg.x && w < rg.y) cols[base + (w - rg.x)] = c;      // (a window the alignment does not overlap: not its business)
                }
                if (p >= 1 && p <= L) {
                    const int w = endw[tb0 + p - 1];
                    if (w >= rg.x && w < rg.y) cole[base + (w - rg.x)] = c;
                }
            }
            pos += __popcll(ng);
        }
    }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void cns_pieces_walk(const mhip_cns_window* __restrict__ win, long long nwin, const int32_t* __restrict__ wtl, int nt,
                                                       const long long* __restrict__ twb, const long long* __restrict__ afirst, const CnsPieceItem* __restrict__ items,
                                                       long long na, long long aln_base, const int2* __restrict__ rng, const long long* __restrict__ abase, long long T,
                                                       const int32_t* __restrict__ cols, const int32_t* __restrict__ cole, int32_t* __restrict__ wcnt,
                                                       const long long* __restrict__ pb, mhip_cns_piece* __restrict__ pieces, long long* __restrict__ bad) {
    const int lane = lane_id();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwin; w += (long long)gridDim.x * 4) {
        const int tl = wtl[w];
        long long a0 = 0, a1 = 0, first_w = 0;
        if (tl >= 0 && tl < nt) {
            a0 = afirst[tl]; a1 = afirst[tl + 1]; first_w = twb[tl];
            if (a0 < 0 || a0 > a1 || a1 > na) { a0 = a1 = 0; if (lane == 0) *bad = 1; }
        }
        const int sb = win[w].sb;
        const long long k0 = EMIT ? pb[w] : 0, k1 = EMIT ? pb[w + 1] : 0;
        long long np = 0;                       // pieces of this window so far
        for (long long r0 = a0; r0 < a1; r0 += 64) {
            const long long a = r0 + lane;
            bool ok = false;
            int col = 0, ncols = 0, sb_out = 0;
            if (a < a1) {
                const int2 rg = rng[a];
                if (w >= rg.x && w < rg.y) {    // se > soff0 && sb < send && n >= 2
                    const CnsPieceItem it = items[a];
                    const long long i = abase[a] + (w - rg.x);
                    if (i < 0 || i >= T) *bad = 1;
                    else {
                        const int n1 = it.aln_size - 1;
                        bool spent = false;     // the previous listed window of the template left the cursor on the last column
                        if (w - 1 >= first_w && w - 1 >= rg.x && i >= 1) {
                            const int pe = cole[i - 1];
                            spent = pe < 0 || pe >= n1;
                        }
                        const int ce = cole[i], cs = cols[i];
                        const int last = ce < 0 ? n1 : ce;
                        col = sb <= it.soff ? 0 : (cs < 0 ? n1 : cs);
                        ncols = last - col + 1;
                        sb_out = max(it.soff, sb);
                        if (last > n1 || col > last) *bad = 1;
                        else ok = !spent;
                    }
                }
            }
            const unsigned long long m = __ballot(ok);
            if (EMIT) {
                const long long k = k0 + np + __popcll(m & lt);
                if (ok && k < k1 && k < T) {
                    int4 rec;
                    rec.x = (int)(aln_base + a); rec.y = col; rec.z = ncols; rec.w = sb_out;
                    *reinterpret_cast<int4*>(pieces + k) = rec;
                }
            }
            np += __popcll(m);
        }
        if (lane == 0) {
            if (EMIT) { if (k0 + np != k1) *bad = 1; }      // not the pieces that were counted: the host refuses the result
            else wcnt[w] = (int32_t)np;
        }
    }
}

}  // namespace

int cns_pieces_launch(mhip_ctx* c, int set, const char* d_str, const CnsPieceItem* items, long long na, long long aln_base, int nt, int t_index0,
                      const long long* afirst, const long long* tb, const mhip_cns_segment* d_seg, long long nseg, const long long* d_segb, long long seg_base,
                      long long win_base, const mhip_cns_window* d_win, long long nwin, CnsPiecesDev* out) {
    *out = CnsPiecesDev();
    if (nwin <= 0 || nt <= 0) return 0;
    if (nwin > 0x7fffffffLL || aln_base + na > 0x7fffffffLL) { mhip_set_error("cns pieces: too many windows or alignments in one batch"); return -1; }
    const long long W = tb[nt] - tb[0];         // template positions of the launch
    if (tb[0] != 0 || W <= 0) { mhip_set_error("cns pieces: the templates' positions must start at 0"); return -1; }
    auto buf = [&](const char* name, size_t bytes, void** p) { return scratch_set(c, name, set, std::max<size_t>(bytes, 16), p); };
    std::vector<long long> head(2 * ((size_t)nt + 1));      // afirst, tb: one upload
    memcpy(head.data(), afirst, sizeof(long long) * ((size_t)nt + 1));
    memcpy(head.data() + (size_t)nt + 1, tb, sizeof(long long) * ((size_t)nt + 1));
    long long *d_head, *d_twb, *d_abase, *d_pb, *d_tot;
    CnsPieceItem* d_items;
    int2* d_rng;
    int32_t *d_acnt, *d_mark, *d_wtl, *d_wcnt, *d_col;
    mhip_cns_piece* d_pieces;
    if (buf("cq_head", sizeof(long long) * head.size(), (void**)&d_head)) return -1;
    if (buf("cq_twb", sizeof(long long) * ((size_t)nt + 1), (void**)&d_twb)) return -1;
    if (buf("cq_items", sizeof(CnsPieceItem) * (size_t)na, (void**)&d_items)) return -1;
    if (buf("cq_rng", sizeof(int2) * (size_t)na, (void**)&d_rng)) return -1;
    if (buf("cq_acnt", sizeof(int32_t) * (size_t)na, (void**)&d_acnt)) return -1;
    if (buf("cq_abase", sizeof(long long) * ((size_t)na + 1), (void**)&d_abase)) return -1;
    if (buf("cq_mark", sizeof(int32_t) * 2 * (size_t)W, (void**)&d_mark)) return -1;
    if (buf("cq_wtl", sizeof(int32_t) * (size_t)nwin, (void**)&d_wtl)) return -1;
    if (buf("cq_wcnt", sizeof(int32_t) * (size_t)nwin, (void**)&d_wcnt)) return -1;
    if (buf("cq_pb", sizeof(long long) * ((size_t)nwin + 1), (void**)&d_pb)) return -1;
    if (buf("cq_tot", 2 * sizeof(long long), (void**)&d_tot)) return -1;      // the bound T; the flag word
    const long long *d_afirst = d_head, *d_tb = d_head + (size_t)nt + 1;
    int32_t *d_startw = d_mark, *d_endw = d_mark + W;
    HIPCHK(hipMemcpyAsync(d_head, head.data(), sizeof(long long) * head.size(), hipMemcpyHostToDevice, c->stream));
    if (na) HIPCHK(hipMemcpyAsync(d_items, items, sizeof(CnsPieceItem) * (size_t)na, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_tot, 0, 2 * sizeof(long long), c->stream));
    HIPCHK(hipMemsetAsync(d_mark, 0xff, sizeof(int32_t) * 2 * (size_t)W, c->stream));
    const unsigned max_grid = (unsigned)c->num_cus * 8;
    auto lanes = [&](long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, (long long)max_grid * 4)); };
    auto waves = [&](long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 3) / 4, (long long)max_grid)); };
    LAUNCH(c, "cns_pieces_tmplwin", cns_pieces_tmplwin, (unsigned)(((long long)nt + 1 + 255) / 256), 256, 0, d_seg, nseg, d_segb, seg_base, win_base, nwin, nt, d_twb, d_tot + 1);
    LAUNCH(c, "cns_pieces_mark", cns_pieces_mark, lanes(nwin), 256, 0, d_win, nwin, d_seg, nseg, seg_base, t_index0, nt, d_tb, d_startw, d_endw, d_wtl, d_tot + 1);
    if (na) LAUNCH(c, "cns_pieces_range", cns_pieces_range, lanes(na), 256, 0, d_items, na, nt, d_twb, d_win, nwin, d_rng, d_acnt, d_tot + 1);
    LAUNCH(c, "cns_pieces_scan", cns_pieces_scan, 1, 1024, 0, d_acnt, na, d_abase, d_tot);
    HIPCHK(hipGetLastError());
    long long tot[2] = {0, 0};
    const double t_wait = wall_now();
    HIPCHK(hipMemcpyAsync(tot, d_tot, 2 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));      // the one wait: T sizes the boundary columns and the pieces (`head` and `items` live until here)
    out->wait_s = wall_now() - t_wait;
    const long long T = tot[0];
    if (tot[1]) { mhip_set_error("cns pieces: the plan's windows, segments and templates do not fit together"); return -1; }
    if (T < 0 || T > na * nwin) { mhip_set_error("cns pieces: inconsistent bound (%lld pairs of %lld alignments and %lld windows)", T, na, nwin); return -1; }
    if (buf("cq_col", sizeof(int32_t) * 2 * (size_t)T, (void**)&d_col)) return -1;
    if (buf("cq_pieces", sizeof(mhip_cns_piece) * (size_t)T, (void**)&d_pieces)) return -1;
    int32_t *d_cols = d_col, *d_cole = d_col + T;
    if (T) {
        HIPCHK(hipMemsetAsync(d_col, 0xff, sizeof(int32_t) * 2 * (size_t)T, c->stream));
        LAUNCH(c, "cns_pieces_cols", cns_pieces_cols, waves(na), 256, 0, d_str, d_items, na, d_rng, d_abase, T, d_tb, nt, d_win, d_startw, d_endw, d_cols, d_cole, d_tot + 1);
    }
    LAUNCH(c, "cns_pieces_count", cns_pieces_walk<false>, waves(nwin), 256, 0, d_win, nwin, d_wtl, nt, d_twb, d_afirst, d_items, na, aln_base, d_rng, d_abase, T, d_cols, d_cole,
           d_wcnt, (const long long*)nullptr, (mhip_cns_piece*)nullptr, d_tot + 1);
    LAUNCH(c, "cns_pieces_scan", cns_pieces_scan, 1, 1024, 0, d_wcnt, nwin, d_pb, (long long*)nullptr);
    LAUNCH(c, "cns_pieces_emit", cns_pieces_walk<true>, waves(nwin), 256, 0, d_win, nwin, d_wtl, nt, d_twb, d_afirst, d_items, na, aln_base, d_rng, d_abase, T, d_cols, d_cole,
           (int32_t*)nullptr, d_pb, d_pieces, d_tot + 1);
    HIPCHK(hipGetLastError());
    out->d_pieces = d_pieces; out->d_pb = d_pb; out->d_items = d_items; out->d_bad = d_tot + 1; out->cap = T;
    return 0;
}

int cns_pieces_debug_launch(mhip_ctx* c, const char* buf, int64_t bytes, const int64_t* off, const int32_t* len, const int32_t* soff, const int32_t* send, int n_pairs,
                            const int32_t* windows, int wstride, int n_windows, CnsPiecesDev* pd, const char** d_buf_out, const mhip_cns_window** d_win_out) {
    *pd = CnsPiecesDev(); *d_buf_out = nullptr; *d_win_out = nullptr;
    if (n_pairs < 0 || n_pairs > 100) { mhip_set_error("cns pieces: %d pairs (at most 100: MAX_CNS_OVLPS)", n_pairs); return -1; }
    if (n_windows < 0) { mhip_set_error("cns pieces: %d windows", n_windows); return -1; }
    long long L = 1;
    std::vector<CnsPieceItem> items((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        if (len[p] < 1) { mhip_set_error("cns pieces: pair %d has len %d (< 1)", p, len[p]); return -1; }
        if (off[p] < 0 || off[p] + 2 * ((int64_t)len[p] + 1) > bytes) { mhip_set_error("cns pieces: pair %d lies outside the buffer", p); return -1; }
        if (soff[p] < 0 || send[p] < 0) { mhip_set_error("cns pieces: pair %d has negative coordinates", p); return -1; }
        const char* s = buf + off[p] + len[p] + 1;
        int64_t bases = 0;
        for (int i = 0; i < len[p]; ++i) bases += s[i] != '-';
        if ((int64_t)send[p] - soff[p] != bases) {
            mhip_set_error("cns pieces: pair %d: send - soff = %lld, but its template string holds %lld bases", p, (long long)send[p] - soff[p], (long long)bases);
            return -1;
        }
        CnsPieceItem& it = items[(size_t)p];
        it.off = (unsigned long long)off[p]; it.aln_size = len[p]; it.soff = soff[p]; it.send = send[p]; it.tl = 0;
        L = std::max<long long>(L, (long long)send[p] + 1);
    }
    std::vector<mhip_cns_window> win((size_t)n_windows);
    for (int w = 0; w < n_windows; ++w) {
        const int32_t sb = windows[(size_t)wstride * w], se = windows[(size_t)wstride * w + 1];
        if (sb < 0 || se < 0) { mhip_set_error("cns pieces: window %d has negative coordinates", w); return -1; }
        if (sb >= se) { mhip_set_error("cns pieces: window %d is not sb < se (%d, %d)", w, sb, se); return -1; }
        if (w && windows[(size_t)wstride * (w - 1) + 1] > sb) { mhip_set_error("cns pieces: windows %d and %d are not ascending and disjoint", w - 1, w); return -1; }
        if (se > 0x3fffffff) { mhip_set_error("cns pieces: window %d ends at %d", w, se); return -1; }
        win[(size_t)w].sb = sb; win[(size_t)w].se = se; win[(size_t)w].cov = wstride > 2 ? windows[(size_t)wstride * w + 2] : 0; win[(size_t)w].segment = 0;
        L = std::max<long long>(L, se);
    }
    if (n_windows == 0) return 0;
    mhip_cns_segment sg;
    sg.template_index = 0; sg.beg = 0; sg.end = (int32_t)L; sg.n_anchors = 0; sg.win_begin = 0; sg.win_end = n_windows;
    const long long segb[2] = {0, 1}, afirst[2] = {0, n_pairs}, tb[2] = {0, L};
    char* d_buf;
    mhip_cns_window* d_win;
    mhip_cns_segment* d_seg;
    long long* d_segb;
    if (c->scratch("cqd_buf", (size_t)std::max<int64_t>(bytes, 1) + 128, (void**)&d_buf)) return -1;
    if (c->scratch("cqd_win", sizeof(mhip_cns_window) * (size_t)n_windows, (void**)&d_win)) return -1;
    if (c->scratch("cqd_seg", sizeof(mhip_cns_segment), (void**)&d_seg)) return -1;
    if (c->scratch("cqd_segb", sizeof(segb), (void**)&d_segb)) return -1;
    if (bytes > 0) HIPCHK(hipMemcpyAsync(d_buf, buf, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_win, win.data(), sizeof(mhip_cns_window) * (size_t)n_windows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_seg, &sg, sizeof(sg), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_segb, segb, sizeof(segb), hipMemcpyHostToDevice, c->stream));
    // (cns_pieces_launch waits for the stream behind these uploads: the host arrays live long enough)
    if (cns_pieces_launch(c, 0, d_buf, items.data(), n_pairs, 0, 1, 0, afirst, tb, d_seg, 1, d_segb, 0, 0, d_win, n_windows, pd)) return -1;
    *d_buf_out = d_buf; *d_win_out = d_win;
    return 0;
}

extern "C" {

// TEST HOOK (tests/test_gpu_cns_pieces.py): the kernels above on one template, host strings and a host window list; see mecat_hip.h
int mhip_debug_cns_pieces(mhip_ctx* c, const char* buf, int64_t bytes, const int64_t* off, const int32_t* len, const int32_t* soff, const int32_t* send, int n_pairs,
                          const int32_t* windows, int n_windows, mhip_cns_piece** out_pieces, int64_t** out_piece_begin) {
    HIPCHK(hipSetDevice(c->device));
    if (!out_pieces || !out_piece_begin) { mhip_set_error("cns pieces: an output pointer is NULL"); return -1; }
    *out_pieces = nullptr; *out_piece_begin = nullptr;
    CnsPiecesDev pd;
    const char* d_buf;
    const mhip_cns_window* d_win;
    if (cns_pieces_debug_launch(c, buf, bytes, off, len, soff, send, n_pairs, windows, 2, n_windows, &pd, &d_buf, &d_win)) return -1;
    struct Out {
        void *pc = nullptr, *pb = nullptr;
        ~Out() { free(pc); free(pb); }
    } o;
    o.pb = calloc((size_t)n_windows + 1, sizeof(int64_t));
    if (!o.pb) { mhip_set_error("out of memory"); return -1; }
    if (n_windows > 0) {
        long long bad = 0;
        HIPCHK(hipMemcpyAsync(o.pb, pd.d_pb, sizeof(long long) * ((size_t)n_windows + 1), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(&bad, pd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const int64_t np = ((int64_t*)o.pb)[n_windows];
        if (bad || np < 0 || np > pd.cap) { mhip_set_error("cns pieces: an index left its array, or the pieces written are not the pieces counted"); return -1; }
        o.pc = malloc(std::max<size_t>(sizeof(mhip_cns_piece) * (size_t)np, 1));
        if (!o.pc) { mhip_set_error("out of memory"); return -1; }
        if (np) HIPCHK(hipMemcpy(o.pc, pd.d_pieces, sizeof(mhip_cns_piece) * (size_t)np, hipMemcpyDeviceToHost));
    } else {
        o.pc = malloc(1);
        if (!o.pc) { mhip_set_error("out of memory"); return -1; }
    }
    *out_pieces = (mhip_cns_piece*)o.pc; *out_piece_begin = (int64_t*)o.pb;
    o.pc = o.pb = nullptr;
    return 0;
}

}  // extern "C"
