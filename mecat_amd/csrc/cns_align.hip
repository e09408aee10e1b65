// cns_align.hip — the mecat2cns re-aligner's entry points.
//
// Replaces ns_banded_sw::Align / dw_in_one_direction / dw / GetAlignment of the reference's src/mecat2cns/dw.cpp (:146-553), which
// mecat2cns calls for up to 200 candidates per template read (mecat_correction.cpp:419-443).  The pipeline of a call, per slice of jobs:
//   cns_caps, cns_scan   every unit's share of the row log and of the block records -> the first record of each unit, the totals
//   cns_forward          dw_extend2<true> (dw_extend2.hip): the d-rows under mecat2cns' block rules, a 16-byte record per row (cns_fwd.h)
//   cns_trace            (cns_trace.hip) one lane per block: the path from the records, the 2-bit columns
//   cns_extend           (cns_extend.hip) the ~0.2 % of the units the forward pass handed over, one per wave with every row kept
// and behind the last slice cns_stitch: dw's merge of the two directions and GetAlignment's trim to the first and last run of four
// matches (:397-480, :495-531).  The row log is sized before it is written; a slice whose log would not fit is halved.
// MECAT_CNS_KERNEL=1 sends every unit through cns_extend instead (the tests compare the two).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "cns_defs.h"
#include "scan.h"

// rows a unit may log: an O(ND) block of size s runs at most max_d = 4 e s rows (dw.cpp:163) and typically (e_q + e_t) s of them; the
// share is 2.7 e of the unit's reach plus one block that fails at max_d (a unit that outgrows it is handed over to cns_extend).
// blocks: one per 256 bases of reach + 4 (a block that contributes advances by about its size; a unit with more blocks than records is
// handed over to cns_extend as well).
__global__ __launch_bounds__(256) void cns_caps(const mhip_offset_t* __restrict__ roffs, const mhip_offset_t* __restrict__ qoffs,
                                                const mhip_aln_job* __restrict__ jobs, int n, double error_rate, uint32_t* __restrict__ caps,
                                                uint32_t* __restrict__ bcaps, int bshift, uint32_t bextra) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u < 2 * n) {
        const mhip_aln_job jb = jobs[u >> 1];
        const int right = u & 1;
        const int qsize = qoffs[jb.qid_local].size, tsize = roffs[jb.sid_local].size;
        const int qs = right ? qsize - jb.qstart : jb.qstart, ts = right ? tsize - jb.sstart : jb.sstart;
        const int ext = (jb.qstart < 0 || jb.sstart < 0) ? 0 : max(min(qs, ts), 0);
        caps[u] = (uint32_t)(2.7 * error_rate * ext) + (uint32_t)(4.0 * error_rate * (CN_SEG + 100)) + 64u;
        bcaps[u] = (uint32_t)(ext >> bshift) + bextra;      // (8, 4 unless the test knob says otherwise)
    }
}
// caps -> first record of every unit, out[m] = total; one workgroup
__global__ __launch_bounds__(1024) void cns_scan(const uint32_t* __restrict__ caps, int m, uint32_t* __restrict__ out, unsigned long long* __restrict__ total) {
    caps += (size_t)blockIdx.x * (size_t)m;            // workgroup b: array b of m counts -> array b of m + 1 positions, total[b]
    out += (size_t)blockIdx.x * ((size_t)m + 1);
    total += blockIdx.x;
    const unsigned long long sum = scan_array_1024<unsigned long long>(      // summed in 64 bits, stored in 32
        m, 0ull, [&](long long i) { return caps[i]; }, [&](long long i, unsigned long long p) { out[i] = (uint32_t)p; });
    if (threadIdx.x == 0) { out[m] = (uint32_t)sum; *total = sum; }
}

__device__ __forceinline__ int cns_op(const uint32_t* __restrict__ w, int c) { return (int)((w[c >> 4] >> ((c & 15) << 1)) & 3u); }

// dw's merge + GetAlignment's trimming (dw.cpp:397-480, 495-531).  Merged column c: c < L.cols -> left op L.cols - 1 - c, else
// right op c - L.cols.  One thread per candidate; the scans stop at the first run of four matches from either end.
__global__ void cns_stitch(const mhip_aln_job* __restrict__ jobs, const CnsDir* __restrict__ dres, const uint32_t* __restrict__ ops,
                           int dir_cols_cap, int n, int min_aln, mhip_cns_result* __restrict__ out, unsigned long long* __restrict__ counters) {
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i0 < n;          // (lanes behind the last candidate redo it and keep nothing: the reductions below want whole waves)
    const int i = live ? i0 : n - 1;
    const size_t dir_words = ((size_t)dir_cols_cap + 15) / 16;
    const CnsDir L = dres[2 * i], R = dres[2 * i + 1];
    const uint32_t* lw = ops + (size_t)(2 * i) * dir_words;
    const uint32_t* rw = lw + dir_words;
    mhip_cns_result r;
    memset(&r, 0, sizeof(r));
    r.left_cols = L.cols; r.right_cols = R.cols;
    r.query_start = jobs[i].qstart - L.qbases; r.query_end = jobs[i].qstart + R.qbases;
    r.target_start = jobs[i].sstart - L.tbases; r.target_end = jobs[i].sstart + R.tbases;
    const int size = L.cols + R.cols;
    r.ins = L.ins + R.ins; r.del = L.del + R.del; r.mat = size - r.ins - r.del;
    bool ok = size >= min_aln;
    int first = 0, last = 0, qrb = 0, trb = 0, qre = 0, tre = 0;
    if (ok) {
        int eit = 0, k;
        for (k = 0; k < size && eit < 4; ++k) {
            const int op = k < L.cols ? cns_op(lw, L.cols - 1 - k) : cns_op(rw, k - L.cols);
            if (op != 1) ++qrb;
            if (op != 2) ++trb;
            if (op == 0) ++eit; else eit = 0;
        }
        if (eit < 4) ok = false;
        first = k - 4; qrb -= 4; trb -= 4;
        if (ok) {
            for (k = size - 1, eit = 0; k >= 0 && eit < 4; --k) {
                const int op = k < L.cols ? cns_op(lw, L.cols - 1 - k) : cns_op(rw, k - L.cols);
                if (op != 1) ++qre;
                if (op != 2) ++tre;
                if (op == 0) ++eit; else eit = 0;
            }
            if (eit < 4) ok = false;
            last = k + 4 + 1; qre -= 4; tre -= 4;
        }
    }
    r.ok = ok ? 1 : 0;
    if (ok) {
        r.qoff = r.query_start + qrb; r.qend = r.query_end - qre;
        r.soff = r.target_start + trb; r.send = r.target_end - tre;
        r.first_col = first; r.last_col = last;
    }
    if (live) out[i] = r;
    // work counters (mecat_hip.h): aligned query bases and alignments like dw_stitch; slot 34: the algorithmic bytes of the job (SURVEY.md
    // §8d's extension figure for an aligner that returns its columns): the two spans at 2 bits a base, the columns at 2 bits, the record
    unsigned long long ab = (ok && live) ? (unsigned long long)(r.query_end - r.query_start) : 0ull, cnt = (ok && live) ? 1ull : 0ull;
    unsigned long long by = !live ? 0ull : (unsigned long long)((r.query_end - r.query_start) + (r.target_end - r.target_start) + size) / 4ull + sizeof(mhip_cns_result);
    for (int o = 32; o; o >>= 1) { ab += __shfl_xor(ab, o); cnt += __shfl_xor(cnt, o); by += __shfl_xor(by, o); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&counters[6], ab); atomicAdd(&counters[7], cnt); atomicAdd(&counters[34], by); }
}

namespace {

int cns_check_args(double error_rate, int dir_cols_cap) {
    if (dir_cols_cap < 16 || (dir_cols_cap & 15)) { mhip_set_error("dir_cols_cap must be a positive multiple of 16"); return -1; }
    if (!(error_rate > 0.0) || error_rate > 0.20) { mhip_set_error("error_rate %.3f outside (0, 0.20]", error_rate); return -1; }
    return 0;
}

// what every stage of a call works on
struct CnsCall {
    const mhip_volume *ref, *reads;
    const mhip_aln_job* jobs;      // device
    int n;
    double error_rate;
    int dir_cols_cap;
    size_t dir_words;              // of a unit's columns in ops
    uint32_t* ops;                 // the caller's, zeroed here
    CnsDir* dres;                  // "cn_dres"
    int* err;                      // the error word (cns_defs.h)
};

int cns_call_buffers(mhip_ctx* c, CnsCall& k) {
    if (c->scratch("cn_dres", sizeof(CnsDir) * 2 * (size_t)k.n, (void**)&k.dres)) return -1;
    if (cns_error_word(c, &k.err)) return -1;
    HIPCHK(hipMemsetAsync(k.err, 0, sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(k.ops, 0, sizeof(uint32_t) * k.dir_words * 2 * (size_t)k.n, c->stream));
    return 0;
}

// the shares of a slice: first row record and first block record of every unit, the two totals, the list of handed-over units
struct CnsShares {
    uint32_t *logbase, *blockbase, *hand;
    unsigned long long rows, blocks;
};
enum { CNS_LOG_FITS = 0, CNS_LOG_HALVE = 1 };      // (-1: refused, the error is set)

// Size the log of jobs [j0, j0 + nj): caps, scan, and the one wait for the host of the slice.  Says whether the log fits the budget and
// 32-bit record numbers, or the slice is to be halved, or (a slice that cannot shrink further) refuses.
int cns_size_log(mhip_ctx* c, const CnsCall& k, int j0, int nj, unsigned long long budget, CnsShares& s) {
    const int nu = 2 * nj;
    uint32_t* d_caps;
    unsigned long long* d_tot;
    if (c->scratch("cnf_totals", 64, (void**)&d_tot)) return -1;
    if (c->scratch("cnf_caps", sizeof(uint32_t) * 2 * (size_t)nu, (void**)&d_caps)) return -1;
    if (c->scratch("cnf_base", sizeof(uint32_t) * 2 * ((size_t)nu + 1), (void**)&s.logbase)) return -1;
    s.blockbase = s.logbase + nu + 1;
    if (c->scratch("cnf_hand", sizeof(uint32_t) * ((size_t)nu + 1), (void**)&s.hand)) return -1;
    HIPCHK(hipMemsetAsync(d_tot, 0, 64, c->stream));
    HIPCHK(hipMemsetAsync(s.hand, 0, sizeof(uint32_t), c->stream));
    int bshift = 8, bextra = 4;
    if (const char* e = getenv("MECAT_CNS_BLOCK_SHARE")) {      // test knob "shift,extra": small shares, so that units run out of block records
        if (sscanf(e, "%d,%d", &bshift, &bextra) != 2 || bshift < 0 || bshift > 30 || bextra < 0) { bshift = 8; bextra = 4; }
    }
    LAUNCH(c, "cns_caps", cns_caps, (nu + 255) / 256, 256, 0, (const mhip_offset_t*)k.ref->d_offs, (const mhip_offset_t*)k.reads->d_offs, k.jobs + j0, nj,
           k.error_rate, d_caps, d_caps + nu, bshift, (uint32_t)bextra);
    LAUNCH(c, "cns_scan", cns_scan, 2, 1024, 0, (const uint32_t*)d_caps, nu, s.logbase, d_tot);      // (two workgroups: rows, block records)
    unsigned long long tot[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    s.rows = tot[0];
    s.blocks = tot[1];
    if ((s.rows * sizeof(CnsRowRec) > budget || s.rows >= (1ull << 32)) && nj > 1024) return CNS_LOG_HALVE;
    if (s.rows >= (1ull << 32)) { mhip_set_error("mecat2cns aligner: the row log of %d jobs does not fit 32-bit record numbers", nj); return -1; }
    if (s.blocks >= (1ull << 32)) { mhip_set_error("mecat2cns aligner: too many block records for %d jobs", nj); return -1; }
    return CNS_LOG_FITS;
}

// forward rows (dw_extend2 under mecat2cns' rules, a 16-byte record per row) -> paths (one lane per block) -> the units the forward
// pass could not finish, redone by cns_extend
int cns_run_slice(mhip_ctx* c, const CnsCall& k, int j0, int nj, const CnsShares& s) {
    const mhip_aln_job* jobs = k.jobs + j0;
    const unsigned int block_cap = (unsigned int)s.blocks;
    CnsFwdArgs a;
    a.error_rate = k.error_rate;
    a.logbase = s.logbase;
    a.blockbase = s.blockbase;
    if (c->scratch("cnf_rowlog", sizeof(CnsRowRec) * ((size_t)s.rows + 8), (void**)&a.rowlog)) return -1;      // (+ 8: cns_trace reads whole groups of four records)
    if (c->scratch("cnf_blocks", sizeof(CnsBlockRec) * (size_t)std::max(block_cap, 1u), (void**)&a.blocks)) return -1;
    HIPCHK(hipMemsetAsync(a.blocks, 0xff, sizeof(CnsBlockRec) * (size_t)block_cap, c->stream));
    a.hand_units = s.hand;
    a.dres = k.dres + 2 * (size_t)j0;
    a.dir_cols_cap = k.dir_cols_cap;
    a.err_flag = k.err;
    uint32_t* ops_slice = k.ops + 2 * (size_t)j0 * k.dir_words;
    if (cns_forward_launch(c, k.ref, k.reads, jobs, nj, a)) return -1;
    if (cns_trace_launch(c, k.ref, k.reads, jobs, a, block_cap, ops_slice, k.err)) return -1;
    // the units the forward pass handed over (0.2 %): cns_extend, which reads their number on the device (nothing waits for the host).
    // (On a second stream beside cns_trace it gained nothing: 118 ms either way on 442 k jobs.)
    const CnsExtendJobs handed = {false, jobs, nj, k.error_rate, 0.3, s.hand};
    if (cns_extend_launch(c, k.ref, k.reads, handed, k.dir_cols_cap, ops_slice, a.dres)) return -1;
    if (getenv("MECAT_TRACE")) {
        unsigned int st = 0;
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(&st, s.hand, sizeof(unsigned int), hipMemcpyDeviceToHost));
        fprintf(stderr, "[mecat_hip] cns re-aligner: jobs %d..%d, row log %.2f GB, room for %u block records, %u of %d units handed over\n", j0, j0 + nj,
                (double)s.rows * sizeof(CnsRowRec) / 1e9, block_cap, st, 2 * nj);
    }
    return 0;
}

// The jobs in slices whose row log stays under MECAT_CNS_LOG_GB (default 24): size the log, halve the slice until it fits, run it.
int cns_run_slices(mhip_ctx* c, const CnsCall& k) {
    const unsigned long long budget = (unsigned long long)(getenv("MECAT_CNS_LOG_GB") ? std::max(1, atoi(getenv("MECAT_CNS_LOG_GB"))) : 24) << 30;
    int slice = std::min(k.n, 1 << 18);
    for (int j0 = 0; j0 < k.n;) {
        const int nj = std::min(slice, k.n - j0);
        CnsShares s;
        const int fit = cns_size_log(c, k, j0, nj, budget, s);
        if (fit < 0) return -1;
        if (fit == CNS_LOG_HALVE) { slice = std::max(1024, nj / 2); continue; }
        if (cns_run_slice(c, k, j0, nj, s)) return -1;
        j0 += nj;
    }
    return 0;
}

int cns_stitch_and_check(mhip_ctx* c, const CnsCall& k, int min_align_size, void* d_results) {
    LAUNCH(c, "cns_stitch", cns_stitch, (k.n + 255) / 256, 256, 0, k.jobs, (const CnsDir*)k.dres, (const uint32_t*)k.ops, k.dir_cols_cap, k.n,
           min_align_size, (mhip_cns_result*)d_results, (unsigned long long*)c->d_counters);
    int err = 0;
    HIPCHK(hipMemcpyAsync(&err, k.err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    if (err == 1) { mhip_set_error("mecat2cns aligner: a direction needed more than dir_cols_cap = %d columns", k.dir_cols_cap); return -1; }
    if (err) { mhip_set_error("mecat2cns aligner: internal error %d (3: a path left its rows; 4: a path missed its end)", err); return -1; }
    return 0;
}

}  // namespace

extern "C" {

int mhip_cns_align_candidates_dev(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, double error_rate,
                                  int min_align_size, int dir_cols_cap, void* d_results, void* d_ops) {
    HIPCHK(hipSetDevice(c->device));
    if (n <= 0) return 0;
    if (cns_check_args(error_rate, dir_cols_cap)) return -1;
    CnsCall k = {ref, reads, (const mhip_aln_job*)d_jobs, n, error_rate, dir_cols_cap, (size_t)dir_cols_cap / 16, (uint32_t*)d_ops, nullptr, nullptr};
    if (cns_call_buffers(c, k)) return -1;
    // MECAT_CNS_KERNEL=1: every unit through cns_extend (one unit per wave, every row kept; the tests compare the two)
    if (getenv("MECAT_CNS_KERNEL") && atoi(getenv("MECAT_CNS_KERNEL")) == 1) {
        const CnsExtendJobs all = {false, d_jobs, n, error_rate, 0.3, nullptr};
        if (cns_extend_launch(c, ref, reads, all, dir_cols_cap, k.ops, k.dres)) return -1;
    } else if (cns_run_slices(c, k)) return -1;
    return cns_stitch_and_check(c, k, min_align_size, d_results);
}

int mhip_cns_align_candidates(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const mhip_aln_job* jobs, int n, double error_rate,
                              int min_align_size, int dir_cols_cap, mhip_cns_result* results, uint32_t* ops) {
    HIPCHK(hipSetDevice(c->device));
    if (n <= 0) return 0;
    void *d_jobs, *d_res, *d_ops;
    const size_t ops_bytes = sizeof(uint32_t) * ((size_t)dir_cols_cap / 16) * 2 * (size_t)n;
    if (c->scratch("cn_jobs", sizeof(mhip_aln_job) * (size_t)n, &d_jobs)) return -1;
    if (c->scratch("cn_res", sizeof(mhip_cns_result) * (size_t)n, &d_res)) return -1;
    if (c->scratch("cn_ops", ops_bytes, &d_ops)) return -1;
    HIPCHK(hipMemcpyAsync(d_jobs, jobs, sizeof(mhip_aln_job) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (mhip_cns_align_candidates_dev(c, ref, reads, d_jobs, n, error_rate, min_align_size, dir_cols_cap, d_res, d_ops)) return -1;
    HIPCHK(hipMemcpyAsync(results, d_res, sizeof(mhip_cns_result) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (ops) HIPCHK(hipMemcpyAsync(ops, d_ops, ops_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
