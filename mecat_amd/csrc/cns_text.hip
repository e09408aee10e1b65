// cns_text.hip — the corrected reads' FASTA text on the device: the loop of reads_correction_can.cpp:44-46 behind a slice's
// cns_reads_letters, while the slice's records and letters are still in device memory.  A cut segment's target is stored once in `seq`
// and the text repeats the overlapping stretches for consecutive records, so the text is made here, from the one stored copy, and the
// host never walks the output again.
//
//   cns_text_size    one lane per record: the record's text length (cns_text.h) — every number is final when cns_reads_records has run.
//   cns_text_scan    one block: the lengths summed (scan.h) — where a record's text goes — and the total the host sizes the output by.
//   cns_text_write   one WAVE per record: lane l writes character l of the header (cns_text_header_char), then the letters are copied
//                    with destination-aligned 16-byte stores, 64 lanes x 16 bytes per pass.  Source and destination sit anywhere mod 16
//                    independently: up to 15 head bytes (a lane each) bring the destination to a 16-byte boundary, every lane then loads
//                    the two aligned 16-byte source words that hold its 16 letters and shifts them into place (the shift is the same
//                    for the whole record), and up to 15 tail bytes and the newline go out a lane each.
// No atomic decides a place: every position is a prefix sum, so the bytes are the same on every run.  Every index that comes from the
// data — seq_begin, size, the text position — is checked before it is used; a failed check sets the flag word (the convention of
// cns_reads.hip's d_bad), as does a record whose bytes written are not the bytes counted, and the host refuses the result.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>

#include "common.h"
#include "cns_text.h"
#include "scan.h"

static_assert(sizeof(mhip_cns_read) == 32, "read records");

namespace {

double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

__device__ __forceinline__ bool cns_text_record_ok(const mhip_cns_read& r, long long seq_bytes) {
    return r.read_id >= 0 && r.range_beg >= 0 && r.range_end >= 0 && r.size >= 0 && r.seq_begin >= 0 && r.seq_begin + (long long)r.size <= seq_bytes;
}

__global__ __launch_bounds__(256) void cns_text_size(const mhip_cns_read* __restrict__ reads, long long n, long long seq_bytes, long long* __restrict__ tlen, long long* __restrict__ bad) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const mhip_cns_read r = reads[i];
        const bool ok = cns_text_record_ok(r, seq_bytes);
        if (!ok) *bad = 1;
        tlen[i] = ok ? cns_text_record_len(r.read_id, r.range_beg, r.range_end, r.size) : 0;
    }
}

// tlen[] (n + 1 entries) -> its exclusive sums in place; tot[0] = bytes of text.  One block of 1024.
__global__ __launch_bounds__(1024) void cns_text_scan(long long* tlen, long long n, long long* __restrict__ tot) {
    const long long bytes = scan_array_1024<long long>(n, 0, [&](long long i) { return tlen[i]; }, [&](long long i, long long p) { tlen[i] = p; });
    if (threadIdx.x == 0) { tlen[n] = bytes; tot[0] = bytes; }
}

// nvec 16-byte words to da[] (aligned) from the bytes that begin Q words and b bytes (0 .. 3) into sa[] (aligned): lane `lane` of 64 takes
// words lane, lane + 64, ..  Output word v is bytes [4 Q + b, 4 Q + b + 16) of the 32 bytes sa[v], sa[v + 1]
template <int Q>
__device__ __forceinline__ void copy_words(const uint4* __restrict__ sa, uint4* __restrict__ da, int nvec, int lane, int b) {
    for (int v = lane; v < nvec; v += 64) {
        const uint4 lo = sa[v], hi = sa[v + 1];
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint4 o;
        o.x = __builtin_amdgcn_alignbyte(w[Q + 1], w[Q], b); o.y = __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], b);
        o.z = __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], b); o.w = __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], b);
        da[v] = o;
    }
}

__global__ __launch_bounds__(256) void cns_text_write(const mhip_cns_read* __restrict__ reads, long long n, const char* __restrict__ seq, long long seq_bytes,
                                                      const long long* __restrict__ tpos, long long text_bytes, char* __restrict__ text, long long* __restrict__ bad) {
    const int lane = lane_id();
    for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (long long)gridDim.x * 4) {
        const mhip_cns_read r = reads[i];
        const long long p0 = tpos[i], p1 = tpos[i + 1];
        bool ok = cns_text_record_ok(r, seq_bytes) && p0 >= 0 && p0 <= p1 && p1 <= text_bytes;
        const int hl = ok ? cns_text_header_len(r.read_id, r.range_beg, r.range_end, r.size) : 0;
        if (ok) ok = p1 - p0 == (long long)hl + r.size + 1;      // the bytes written below are the bytes counted
        if (!ok) { if (lane == 0) *bad = 1; continue; }
        if (lane < hl) text[p0 + lane] = cns_text_header_char(r.read_id, r.range_beg, r.range_end, r.size, lane);
        char* d = text + p0 + hl;
        const char* s = seq + r.seq_begin;
        const int head = min(r.size, (int)((16u - (unsigned)((uintptr_t)d & 15u)) & 15u));
        if (lane < head) d[lane] = s[lane];
        d += head; s += head;
        const int rem = r.size - head, nvec = rem >> 4, tail = rem & 15;
        const int m = __builtin_amdgcn_readfirstlane((int)((uintptr_t)s & 15u));      // (the same on every lane: one branch for the wave)
        // (the buffer begins on a 16-byte boundary and has 16 bytes of room behind seq_bytes: sa[v + 1] ends at most 16 - m bytes behind it)
        const uint4* __restrict__ sa = (const uint4*)(s - m);
        uint4* __restrict__ da = (uint4*)d;
        switch (m >> 2) {
            case 0: copy_words<0>(sa, da, nvec, lane, m & 3); break;
            case 1: copy_words<1>(sa, da, nvec, lane, m & 3); break;
            case 2: copy_words<2>(sa, da, nvec, lane, m & 3); break;
            default: copy_words<3>(sa, da, nvec, lane, m & 3); break;
        }
        if (lane < tail) d[16 * nvec + lane] = s[16 * nvec + lane];
        if (lane == 0) d[rem] = '\n';
    }
}

const char* const TEXT_BAD = "cns text: a record leaves the letters or holds a negative number, or the bytes written are not the bytes counted";

}  // namespace

int cns_text_launch(mhip_ctx* c, int set, const mhip_cns_read* d_reads, long long nreads, const char* d_seq, long long seq_bytes, CnsTextDev* out) {
    *out = CnsTextDev();
    if (nreads <= 0) return 0;
    if (((uintptr_t)d_seq & 15u) != 0) { mhip_set_error("cns text: the letters do not begin on a 16-byte boundary"); return -1; }
    long long *d_pos, *d_tot;
    if (scratch_set(c, "ct_pos", set, sizeof(long long) * ((size_t)nreads + 1), (void**)&d_pos)) return -1;
    if (scratch_set(c, "ct_tot", set, 2 * sizeof(long long), (void**)&d_tot)) return -1;      // bytes of text, the flag word
    HIPCHK(hipMemsetAsync(d_tot, 0, 2 * sizeof(long long), c->stream));
    long long* d_bad = d_tot + 1;
    const unsigned max_grid = (unsigned)c->num_cus * 8;
    const unsigned grid_s = (unsigned)std::max<long long>(1, std::min<long long>((nreads + 255) / 256, max_grid));
    LAUNCH(c, "cns_text_size", cns_text_size, grid_s, 256, 0, d_reads, nreads, seq_bytes, d_pos, d_bad);
    LAUNCH(c, "cns_text_scan", cns_text_scan, 1, 1024, 0, d_pos, nreads, d_tot);
    HIPCHK(hipGetLastError());
    long long tot[2] = {0, 0};
    const double t_wait = wall_now();
    HIPCHK(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));      // the one wait: the total sizes the output
    out->wait_s = wall_now() - t_wait;
    if (tot[1]) { mhip_set_error("%s", TEXT_BAD); return -1; }
    if (tot[0] < 10 * nreads) { mhip_set_error("cns text: inconsistent total (%lld bytes for %lld records)", tot[0], nreads); return -1; }
    char* d_text;
    if (scratch_set(c, "ct_text", set, (size_t)tot[0] + 16, (void**)&d_text)) return -1;
    const unsigned grid_w = (unsigned)std::max<long long>(1, std::min<long long>((nreads + 3) / 4, max_grid));
    LAUNCH(c, "cns_text_write", cns_text_write, grid_w, 256, 0, d_reads, nreads, d_seq, seq_bytes, d_pos, tot[0], d_text, d_bad);
    HIPCHK(hipGetLastError());
    out->d_text = d_text; out->d_bad = d_bad; out->bytes = tot[0];
    return 0;
}

extern "C" {

// TEST HOOK (tests/test_gpu_cns_text.py): the kernels above on host-supplied records; see mecat_hip.h
int mhip_debug_cns_text(mhip_ctx* c, const mhip_cns_read* reads, int64_t n, const char* seq, int64_t seq_bytes, char** out_text, int64_t* out_bytes) {
    HIPCHK(hipSetDevice(c->device));
    if (!out_text || !out_bytes) { mhip_set_error("cns text: an output pointer is NULL"); return -1; }
    *out_text = nullptr; *out_bytes = 0;
    if (n < 0 || seq_bytes < 0 || (n > 0 && !reads) || (seq_bytes > 0 && !seq)) { mhip_set_error("cns text: %lld records, %lld letters, or a NULL array", (long long)n, (long long)seq_bytes); return -1; }
    for (int64_t i = 0; i < n; ++i) {
        const mhip_cns_read& r = reads[i];
        if (r.size < 0 || r.seq_begin < 0 || r.seq_begin + r.size > seq_bytes) { mhip_set_error("cns text: record %lld leaves the letters", (long long)i); return -1; }
        if (r.read_id < 0 || r.range_beg < 0 || r.range_end < 0) { mhip_set_error("cns text: record %lld holds a negative number", (long long)i); return -1; }
    }
    CnsTextDev td;
    if (n > 0) {
        mhip_cns_read* d_reads; char* d_seq;
        if (c->scratch("ctd_reads", sizeof(mhip_cns_read) * (size_t)n, (void**)&d_reads)) return -1;
        if (c->scratch("ctd_seq", (size_t)seq_bytes + 16, (void**)&d_seq)) return -1;
        HIPCHK(hipMemcpyAsync(d_reads, reads, sizeof(mhip_cns_read) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        if (seq_bytes) HIPCHK(hipMemcpyAsync(d_seq, seq, (size_t)seq_bytes, hipMemcpyHostToDevice, c->stream));
        if (cns_text_launch(c, 0, d_reads, n, d_seq, seq_bytes, &td)) return -1;
    }
    char* text = (char*)malloc(std::max<size_t>((size_t)td.bytes, 1));
    if (!text) { mhip_set_error("out of memory"); return -1; }
    long long bad = 0;
    hipError_t e = hipSuccess;
    if (td.bytes) e = hipMemcpyAsync(text, td.d_text, (size_t)td.bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && td.d_bad) e = hipMemcpyAsync(&bad, td.d_bad, sizeof(long long), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || bad) {
        free(text);
        if (bad) mhip_set_error("%s", TEXT_BAD); else mhip_set_error("cns text: %s", hipGetErrorString(e));
        return -1;
    }
    *out_text = text; *out_bytes = td.bytes;
    return 0;
}

}  // extern "C"
