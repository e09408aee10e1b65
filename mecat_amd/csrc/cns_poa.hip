// cns_poa.hip — the POA consensus of the listed windows on the device: meap_cns_one_indel (mecat2cns/mecat_correction.cpp:62-78) for
// every window of a slice, behind the slice's pieces (cns_pieces.hip) while its strings are still in device memory.  The graph routine
// is cns_poa.h, the one the host build is pinned to the reference with; a kernel here is that routine plus memory management.
//
//   cns_poa_bound   one LANE per window: reads the columns of the window's pieces once and counts their insertion columns and addEdge
//                   calls (cns_poa_count), which give the routine's exact capacities — nodes = blen + 2 + insertions, edges = blen + 1 +
//                   calls — its workspace in words, and nodes - 2 as the bound on the consensus' length.  A record that leaves its
//                   alignment sets the flag word and the window is skipped.
//   cns_poa_scan    exclusive 64-bit sums (one block): where a window's bounded output starts, which number a large window has, where
//                   its workspace starts.
//   cns_poa_small   windows whose workspace fits a slot of CNS_POA_SLOT_WORDS words: one window per LANE, a slot per lane in GLOBAL
//                   memory.  (Not LDS: a graph of 100 edges is 4 KB, so the 160 KB of a CU would hold a few dozen lanes; the slots of
//                   a resident grid stay in L2 / MALL instead.)  Lanes of a wave diverge; accepted.
//   cns_poa_large   the rest, one window per lane as well, each with a workspace of its own size in a global buffer.  The large windows
//                   are taken in CHUNKS: window i with workspace prefix P[i] belongs to chunk P[i] / budget and lies at P[i] mod budget
//                   in a buffer of budget + (the largest workspace) words; one launch per chunk, lanes find the chunk's windows by
//                   binary search in P.  MECAT_CNS_POA_CHUNK_BYTES sets the budget (default 1 GiB).
//   cns_poa_gather  lengths summed by cns_poa_scan give cns_begin; one lane per window copies its string to its place.
// Every window gets its answer here.  A return code of the routine other than 0 means its bound was wrong or a piece leaves the
// backbone: the flag word (the convention of cns_pieces.hip's d_bad) is set and the host refuses the result.
// The host WAITS once per launch, for the three totals that size the buffers.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "common.h"
#include "cns_pieces.h"
#include "cns_poa.h"
#include "cns_poa_dev.h"
#include "scan.h"

namespace {

double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct DevPieces {
    const char* str;
    const CnsPieceItem* items;
    long long aln_base;
    const mhip_cns_piece* pc;      // the window's first record
    __device__ void operator()(int k, const char** q, const char** t, int* ncols, int* sb_out) const {
        const mhip_cns_piece r = pc[k];
        const CnsPieceItem it = items[(long long)r.aln - aln_base];
        *q = str + it.off + r.col;
        *t = *q + it.aln_size + 1;
        *ncols = r.ncols;
        *sb_out = r.sb_out;
    }
};

// per window: nodes, edges (0, 0: skipped), words of workspace, bound on the output
__global__ __launch_bounds__(256) void cns_poa_bound(const mhip_cns_window* __restrict__ win, long long nwin, const mhip_cns_piece* __restrict__ pieces,
                                                     const long long* __restrict__ pb, long long pcap, const CnsPieceItem* __restrict__ items, long long na, long long aln_base,
                                                     const char* __restrict__ str, int2* __restrict__ caps, long long* __restrict__ obound, long long* __restrict__ islarge,
                                                     long long* __restrict__ lwords, long long* __restrict__ bad) {
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < nwin; w += (long long)gridDim.x * 256) {
        const mhip_cns_window x = win[w];
        const long long p0 = pb[w], p1 = pb[w + 1];
        long long nodes = 0, edges = 0;
        bool ok = x.sb >= 0 && x.sb < x.se && p0 >= 0 && p0 <= p1 && p1 <= pcap && x.cov >= 0;
        if (ok) {
            long long ins = 0, calls = 0;
            for (long long k = p0; k < p1 && ok; ++k) {
                const mhip_cns_piece r = pieces[k];
                const long long a = (long long)r.aln - aln_base;
                if (a < 0 || a >= na) { ok = false; break; }
                const CnsPieceItem it = items[a];
                if (r.col < 0 || r.ncols < 1 || (long long)r.col + r.ncols > it.aln_size || r.sb_out < x.sb || r.sb_out > x.se) { ok = false; break; }
                const char* q = str + it.off + r.col;
                cns_poa_count(q, q + it.aln_size + 1, r.ncols, &ins, &calls);
            }
            const long long blen = (long long)x.se - x.sb + 1;
            nodes = blen + 2 + ins; edges = blen + 1 + calls;
            if (nodes > 0x3fffffffLL || edges > 0x3fffffffLL) ok = false;
        }
        if (!ok) { *bad = 1; nodes = edges = 0; }
        const long long words = cns_poa_words(nodes, edges);
        const bool large = words > CNS_POA_SLOT_WORDS;
        caps[w] = make_int2((int)nodes, (int)edges);
        obound[w] = ok ? nodes - 2 : 0;
        islarge[w] = large;
        lwords[w] = large ? words : 0;
    }
}

// out[i] = v[0] + .. + v[i - 1] for i <= n; IN PLACE is fine (out == v; then v needs n + 1 entries).  One block of 1024.  *vmax: the largest v
__global__ __launch_bounds__(1024) void cns_poa_scan(const long long* v, long long n, long long* out, long long* __restrict__ total, long long* __restrict__ vmax) {
    __shared__ long long wmax[16];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    long long mx = 0;
    const long long run = scan_array_1024<long long>(
        n, 0, [&](long long i) { const long long x = v[i]; mx = max(mx, x); return x; }, [&](long long i, long long p) { out[i] = p; });
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
    if (lane == 0) wmax[w] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 16; ++k) mx = max(mx, wmax[k]);
        out[n] = run;
        if (total) *total = run;
        if (vmax) *vmax = mx;
    }
}

// large window number i -> its window, and its workspace prefix moved to the list
__global__ __launch_bounds__(256) void cns_poa_list(long long nwin, const int2* __restrict__ caps, const long long* __restrict__ lidx, const long long* __restrict__ lpre,
                                                    long long nlarge, int32_t* __restrict__ lwin, long long* __restrict__ P) {
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w <= nwin; w += (long long)gridDim.x * 256) {
        if (w == nwin) { P[nlarge] = lpre[nwin]; continue; }
        const int2 cp = caps[w];
        if (cns_poa_words(cp.x, cp.y) <= CNS_POA_SLOT_WORDS) continue;
        const long long i = lidx[w];
        if (i < 0 || i >= nlarge) continue;
        lwin[i] = (int32_t)w;
        P[i] = lpre[w];
    }
}

__device__ __forceinline__ void poa_one(long long w, const mhip_cns_window* __restrict__ win, const int2* __restrict__ caps, const DevPieces& base, const long long* __restrict__ pb,
                                        int32_t* ws, const long long* __restrict__ obegin, char* __restrict__ tmp, int32_t* __restrict__ len, long long* __restrict__ bad) {
    const mhip_cns_window x = win[w];
    const int2 cp = caps[w];
    DevPieces get = base;
    get.pc = base.pc + pb[w];
    int32_t n = 0;
    const int rc = cns_poa_window(x.sb, x.se, x.cov, get, (int)(pb[w + 1] - pb[w]), ws, cp.x, cp.y, tmp + obegin[w], cp.x - 2, &n, (CnsPoaStats*)nullptr);
    if (rc) { *bad = 1; n = 0; }
    len[w] = n;
}

__global__ __launch_bounds__(256) void cns_poa_small(const mhip_cns_window* __restrict__ win, long long nwin, const int2* __restrict__ caps, DevPieces base,
                                                     const long long* __restrict__ pb, int32_t* __restrict__ slots, const long long* __restrict__ obegin, char* __restrict__ tmp,
                                                     int32_t* __restrict__ len, long long* __restrict__ bad) {
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    int32_t* ws = slots + lane * CNS_POA_SLOT_WORDS;
    for (long long w = lane; w < nwin; w += (long long)gridDim.x * 256) {
        const int2 cp = caps[w];
        if (cp.x == 0) { len[w] = 0; continue; }                              // refused by cns_poa_bound
        if (cns_poa_words(cp.x, cp.y) > CNS_POA_SLOT_WORDS) continue;          // cns_poa_large's
        poa_one(w, win, caps, base, pb, ws, obegin, tmp, len, bad);
    }
}

__global__ __launch_bounds__(256) void cns_poa_large(const mhip_cns_window* __restrict__ win, const int2* __restrict__ caps, DevPieces base, const long long* __restrict__ pb,
                                                     const int32_t* __restrict__ lwin, const long long* __restrict__ P, long long nlarge, long long chunk, long long budget,
                                                     long long buf_words, long long nwin, int32_t* __restrict__ buf, const long long* __restrict__ obegin, char* __restrict__ tmp,
                                                     int32_t* __restrict__ len, long long* __restrict__ bad) {
    // the chunk's windows: prefixes in [chunk * budget, (chunk + 1) * budget)
    long long lo = 0, hi = nlarge;
    while (lo < hi) { const long long m = (lo + hi) >> 1; if (P[m] >= chunk * budget) hi = m; else lo = m + 1; }
    const long long first = lo;
    hi = nlarge;
    while (lo < hi) { const long long m = (lo + hi) >> 1; if (P[m] >= (chunk + 1) * budget) hi = m; else lo = m + 1; }
    const long long last = lo;
    for (long long i = first + (long long)blockIdx.x * 256 + threadIdx.x; i < last; i += (long long)gridDim.x * 256) {
        const long long w = lwin[i];
        const long long o = P[i] - chunk * budget;
        if (w < 0 || w >= nwin) { *bad = 1; continue; }
        const int2 cp = caps[w];
        if (o < 0 || o + cns_poa_words(cp.x, cp.y) > buf_words) { *bad = 1; len[w] = 0; continue; }
        poa_one(w, win, caps, base, pb, buf + o, obegin, tmp, len, bad);
    }
}

__global__ __launch_bounds__(256) void cns_poa_widen(const int32_t* __restrict__ len, long long nwin, long long* __restrict__ len64) {
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < nwin; w += (long long)gridDim.x * 256) len64[w] = len[w];
}

__global__ __launch_bounds__(256) void cns_poa_gather(long long nwin, const int32_t* __restrict__ len, const long long* __restrict__ obegin, const char* __restrict__ tmp,
                                                      const long long* __restrict__ cb, long long cap, char* __restrict__ cns, long long* __restrict__ bad) {
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < nwin; w += (long long)gridDim.x * 256) {
        const long long n = len[w], d = cb[w], s = obegin[w];
        if (n < 0 || d < 0 || d + n > cap || n > obegin[w + 1] - s) { *bad = 1; continue; }
        for (long long i = 0; i < n; ++i) cns[d + i] = tmp[s + i];
    }
}

long long g_last[2] = {0, 0};      // the last launch's large windows and chunks (mhip_debug_cns_poa_last)

long long chunk_budget_words() {
    long long bytes = (long long)1 << 30;
    if (const char* e = getenv("MECAT_CNS_POA_CHUNK_BYTES")) bytes = std::max<long long>(4, atoll(e));
    return std::max<long long>(1, bytes / 4);
}

}  // namespace

int cns_poa_launch(mhip_ctx* c, int set, const char* d_str, const CnsPiecesDev& pd, long long na, long long aln_base, const mhip_cns_window* d_win, long long nwin,
                   CnsPoaDev* out) {
    *out = CnsPoaDev();
    if (nwin <= 0) return 0;
    if (nwin > 0x7fffffffLL) { mhip_set_error("cns poa: too many windows in one batch"); return -1; }
    auto buf = [&](const char* name, size_t bytes, void** p) { return scratch_set(c, name, set, std::max<size_t>(bytes, 16), p); };
    const size_t n1 = (size_t)nwin + 1;
    int2* d_caps;
    long long *d_ob, *d_li, *d_lw, *d_tot, *d_cb;
    int32_t* d_len;
    if (buf("co_caps", sizeof(int2) * (size_t)nwin, (void**)&d_caps)) return -1;
    if (buf("co_ob", sizeof(long long) * n1, (void**)&d_ob)) return -1;
    if (buf("co_li", sizeof(long long) * n1, (void**)&d_li)) return -1;
    if (buf("co_lw", sizeof(long long) * n1, (void**)&d_lw)) return -1;
    if (buf("co_cb", sizeof(long long) * n1, (void**)&d_cb)) return -1;
    if (buf("co_len", sizeof(int32_t) * (size_t)nwin, (void**)&d_len)) return -1;
    if (buf("co_tot", 5 * sizeof(long long), (void**)&d_tot)) return -1;      // output bound, large windows, their words, the largest, the flag word
    HIPCHK(hipMemsetAsync(d_tot, 0, 5 * sizeof(long long), c->stream));
    HIPCHK(hipMemsetAsync(d_len, 0, sizeof(int32_t) * (size_t)nwin, c->stream));
    const unsigned max_grid = (unsigned)c->num_cus * 8;
    auto lanes = [&](long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, (long long)max_grid * 4)); };
    long long* d_bad = d_tot + 4;
    LAUNCH(c, "cns_poa_bound", cns_poa_bound, lanes(nwin), 256, 0, d_win, nwin, pd.d_pieces, pd.d_pb, pd.cap, pd.d_items, na, aln_base, d_str, d_caps, d_ob, d_li, d_lw, d_bad);
    LAUNCH(c, "cns_poa_scan", cns_poa_scan, 1, 1024, 0, d_ob, nwin, d_ob, d_tot, (long long*)nullptr);
    LAUNCH(c, "cns_poa_scan", cns_poa_scan, 1, 1024, 0, d_li, nwin, d_li, d_tot + 1, (long long*)nullptr);
    LAUNCH(c, "cns_poa_scan", cns_poa_scan, 1, 1024, 0, d_lw, nwin, d_lw, d_tot + 2, d_tot + 3);
    HIPCHK(hipGetLastError());
    long long tot[5] = {0, 0, 0, 0, 0};
    const double t_wait = wall_now();
    HIPCHK(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));      // the one wait: the totals size the output, the slots and the large windows' buffer
    out->wait_s = wall_now() - t_wait;
    const long long OB = tot[0], nlarge = tot[1], lwords = tot[2], lmax = tot[3];
    if (tot[4]) { mhip_set_error("cns poa: a piece leaves its alignment or its window"); return -1; }
    if (OB < 0 || nlarge < 0 || nlarge > nwin || lwords < 0 || lmax < 0 || lmax > lwords) { mhip_set_error("cns poa: inconsistent bounds"); return -1; }
    char *d_tmp, *d_cns;
    if (buf("co_tmp", (size_t)OB, (void**)&d_tmp)) return -1;
    if (buf("co_cns", (size_t)OB, (void**)&d_cns)) return -1;
    DevPieces base = {d_str, pd.d_items, aln_base, pd.d_pieces};
    const long long nsmall = nwin - nlarge;
    if (nsmall > 0) {
        const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((nwin + 255) / 256, (long long)c->num_cus * 2));
        int32_t* d_slots;
        if (buf("co_slots", sizeof(int32_t) * (size_t)grid * 256 * CNS_POA_SLOT_WORDS, (void**)&d_slots)) return -1;
        LAUNCH(c, "cns_poa_small", cns_poa_small, grid, 256, 0, d_win, nwin, d_caps, base, pd.d_pb, d_slots, d_ob, d_tmp, d_len, d_bad);
    }
    int nchunks = 0;
    if (nlarge > 0) {
        const long long budget = chunk_budget_words();
        const long long buf_words = std::min(lwords, budget + lmax);
        int32_t *d_lwin, *d_lbuf;
        long long* d_P;
        if (buf("co_lwin", sizeof(int32_t) * (size_t)nlarge, (void**)&d_lwin)) return -1;
        if (buf("co_P", sizeof(long long) * ((size_t)nlarge + 1), (void**)&d_P)) return -1;
        if (buf("co_lbuf", sizeof(int32_t) * (size_t)buf_words, (void**)&d_lbuf)) return -1;
        LAUNCH(c, "cns_poa_list", cns_poa_list, lanes(nwin + 1), 256, 0, nwin, d_caps, d_li, d_lw, nlarge, d_lwin, d_P);
        const long long nch = (lwords + budget - 1) / budget;
        if (nch > 1000000) { mhip_set_error("cns poa: MECAT_CNS_POA_CHUNK_BYTES is too small for %lld words of workspace", lwords); return -1; }
        const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((nlarge + 255) / 256, (long long)c->num_cus * 2));
        for (long long k = 0; k < nch; ++k)
            LAUNCH(c, "cns_poa_large", cns_poa_large, grid, 256, 0, d_win, d_caps, base, pd.d_pb, d_lwin, d_P, nlarge, k, budget, buf_words, nwin, d_lbuf, d_ob, d_tmp, d_len, d_bad);
        nchunks = (int)nch;
    }
    LAUNCH(c, "cns_poa_widen", cns_poa_widen, lanes(nwin), 256, 0, d_len, nwin, d_cb);
    LAUNCH(c, "cns_poa_scan", cns_poa_scan, 1, 1024, 0, d_cb, nwin, d_cb, (long long*)nullptr, (long long*)nullptr);
    LAUNCH(c, "cns_poa_gather", cns_poa_gather, lanes(nwin), 256, 0, nwin, d_len, d_ob, d_tmp, d_cb, OB, d_cns, d_bad);
    HIPCHK(hipGetLastError());
    g_last[0] = nlarge; g_last[1] = nchunks;
    out->d_cns = d_cns; out->d_cb = d_cb; out->d_bad = d_bad; out->cap = OB; out->nlarge = nlarge; out->nchunks = nchunks;
    return 0;
}

extern "C" {

int64_t mhip_cns_poa_small_words(void) { return CNS_POA_SLOT_WORDS; }

// TEST HOOK: how the last POA launch of the process was split
void mhip_debug_cns_poa_last(int64_t* out) { out[0] = g_last[0]; out[1] = g_last[1]; }

// TEST HOOK (tests/test_gpu_cns_poa.py): the piece kernels and then the kernels above on one template; see mecat_hip.h
int mhip_debug_cns_poa(mhip_ctx* c, const char* buf, int64_t bytes, const int64_t* off, const int32_t* len, const int32_t* soff, const int32_t* send, int n_pairs,
                       const int32_t* windows, int n_windows, char** out_cns, int64_t** out_cns_begin) {
    HIPCHK(hipSetDevice(c->device));
    if (!out_cns || !out_cns_begin) { mhip_set_error("cns poa: an output pointer is NULL"); return -1; }
    *out_cns = nullptr; *out_cns_begin = nullptr;
    for (int w = 0; w < n_windows; ++w)
        if (windows[3 * (size_t)w + 2] < 0) { mhip_set_error("cns poa: window %d has cov %d (< 0)", w, windows[3 * (size_t)w + 2]); return -1; }
    CnsPiecesDev pd;
    const char* d_buf;
    const mhip_cns_window* d_win;
    if (cns_pieces_debug_launch(c, buf, bytes, off, len, soff, send, n_pairs, windows, 3, n_windows, &pd, &d_buf, &d_win)) return -1;
    struct Out {
        void *cns = nullptr, *cb = nullptr;
        ~Out() { free(cns); free(cb); }
    } o;
    o.cb = calloc((size_t)std::max(n_windows, 0) + 1, sizeof(int64_t));
    if (!o.cb) { mhip_set_error("out of memory"); return -1; }
    int64_t total = 0;
    if (n_windows > 0) {
        CnsPoaDev od;
        if (cns_poa_launch(c, 0, d_buf, pd, n_pairs, 0, d_win, n_windows, &od)) return -1;
        long long bad[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(o.cb, od.d_cb, sizeof(long long) * ((size_t)n_windows + 1), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(&bad[0], od.d_bad, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(&bad[1], pd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        total = ((int64_t*)o.cb)[n_windows];
        if (bad[1]) { mhip_set_error("cns pieces: an index left its array, or the pieces written are not the pieces counted"); return -1; }
        if (bad[0] || total < 0 || total > od.cap) { mhip_set_error("cns poa: a window's graph left its workspace bound, or a piece leaves its backbone"); return -1; }
        o.cns = malloc(std::max<size_t>((size_t)total, 1));
        if (!o.cns) { mhip_set_error("out of memory"); return -1; }
        if (total) HIPCHK(hipMemcpy(o.cns, od.d_cns, (size_t)total, hipMemcpyDeviceToHost));
    } else {
        o.cns = malloc(1);
        if (!o.cns) { mhip_set_error("out of memory"); return -1; }
    }
    *out_cns = (char*)o.cns; *out_cns_begin = (int64_t*)o.cb;
    o.cns = o.cb = nullptr;
    return 0;
}

}  // extern "C"
