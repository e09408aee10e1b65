// xd_order.hip — longest first, for the X-drop aligner's launch (xalign.hip).  The waves pull units from a cursor; a unit is as long as
// the shorter of the two sequences on its side of the start point allows (its reach), and the kernel ends with its last unit: handing the
// JOBS out in descending order of their longer side's reach takes the long units off the kernel's tail (-3 % on 134 k ONT-style jobs).
// The sort is stable and by job — the two units of a job and the jobs of one read stay neighbours, which is worth more than the order
// itself (a per-unit scatter lost 4 % to cache misses): one stable counting sort over 64 bins of 1 kb in two passes, every thread
// counting and then placing a contiguous part of the jobs.
#include <algorithm>

#include "common.h"
#include "scan.h"
#include "xd_defs.h"

#define XO_BINS 64
__device__ __forceinline__ int xo_bin(const mhip_aln_job& jb, const mhip_offset_t* __restrict__ roffs, const mhip_offset_t* __restrict__ qoffs) {
    int reach = 0;
    if (jb.qstart >= 0 && jb.sstart >= 0) {
        const int qsize = qoffs[jb.qid_local].size, tsize = roffs[jb.sid_local].size;
        reach = max(min(qsize - jb.qstart, tsize - jb.sstart), min(jb.qstart, jb.sstart));
    }
    return XO_BINS - 1 - min(max(reach, 0) >> 10, XO_BINS - 1);          // bin 0 = the longest
}
// pass 1 (PLACE = false): jobs per bin of every workgroup's stretch -> cnt[bin][workgroup]; xo_scan: exclusive prefix over (bin, workgroup);
// pass 2 (PLACE = true): every thread places its own contiguous part of the stretch behind the threads before it, bin by bin.
#define XO_THREADS 256
template <bool PLACE>
__global__ __launch_bounds__(XO_THREADS) void xo_order_jobs(const mhip_aln_job* __restrict__ jobs, int n, const mhip_offset_t* __restrict__ roffs,
                                                          const mhip_offset_t* __restrict__ qoffs, unsigned int* __restrict__ cnt, unsigned int* __restrict__ order) {
    __shared__ uint16_t tc[XO_BINS][XO_THREADS];        // jobs of thread t in bin b (a thread's part is < 65 536 jobs: the host checks)
    __shared__ unsigned int wsum[XO_THREADS / 64];
    __shared__ unsigned int base;
    const int t = (int)threadIdx.x, G = (int)gridDim.x;
    const int per_block = (n + G - 1) / G, b0 = min(n, (int)blockIdx.x * per_block), b1 = min(n, b0 + per_block);
    const int per = (b1 - b0 + XO_THREADS - 1) / XO_THREADS, lo = min(b1, b0 + t * per), hi = min(b1, lo + per);
    for (int b = 0; b < XO_BINS; ++b) tc[b][t] = 0;
    for (int i = lo; i < hi; ++i) ++tc[xo_bin(jobs[i], roffs, qoffs)][t];
    __syncthreads();
    unsigned int mypos[XO_BINS];
#pragma unroll
    for (int b = 0; b < XO_BINS; ++b) {
        if (t == 0) base = PLACE ? cnt[(size_t)b * G + blockIdx.x] : 0u;
        const unsigned int c = tc[b][t];
        unsigned int incl = c;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int v = __shfl_up(incl, o);
            if ((t & 63) >= o) incl += v;
        }
        if ((t & 63) == 63) wsum[t >> 6] = incl;
        __syncthreads();
        unsigned int before = base;
        for (int k = 0; k < (t >> 6); ++k) before += wsum[k];
        mypos[b] = before + incl - c;
        if (!PLACE && t == XO_THREADS - 1) cnt[(size_t)b * G + blockIdx.x] = before + incl;
        __syncthreads();
    }
    if (!PLACE) return;
    for (int i = lo; i < hi; ++i) {
        const int b = xo_bin(jobs[i], roffs, qoffs);
        unsigned int p = 0;
#pragma unroll
        for (int k = 0; k < XO_BINS; ++k) if (k == b) p = mypos[k]++;        // (registers: no dynamic indexing)
        order[p] = (unsigned int)i;
    }
}
__global__ __launch_bounds__(1024) void xo_scan(unsigned int* __restrict__ cnt, int m) {      // counts -> first positions, in place; one workgroup
    scan_array_1024<unsigned int>(m, 0u, [&](long long i) { return cnt[i]; }, [&](long long i, unsigned int p) { cnt[i] = p; });
}

int xd_order_jobs(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, int waves, unsigned int** d_order) {
    *d_order = nullptr;
    if ((size_t)n <= (size_t)waves) return 0;
    const int G = (int)std::min<size_t>((size_t)c->num_cus, ((size_t)n + 4095) / 4096 + 1);      // (a thread's part stays far below 65 536 jobs)
    unsigned int *d_cnt, *d_ord;
    if (c->scratch("xo_cnt", sizeof(unsigned int) * XO_BINS * (size_t)G, (void**)&d_cnt)) return -1;
    if (c->scratch("xo_order", sizeof(unsigned int) * (size_t)n, (void**)&d_ord)) return -1;
    if ((size_t)n / ((size_t)G * XO_THREADS) >= 65535) return 0;
    LAUNCH(c, "xo_count", xo_order_jobs<false>, G, XO_THREADS, 0, (const mhip_aln_job*)d_jobs, n, (const mhip_offset_t*)ref->d_offs, (const mhip_offset_t*)reads->d_offs, d_cnt, d_ord);
    LAUNCH(c, "xo_scan", xo_scan, 1, 1024, 0, d_cnt, XO_BINS * G);
    LAUNCH(c, "xo_place", xo_order_jobs<true>, G, XO_THREADS, 0, (const mhip_aln_job*)d_jobs, n, (const mhip_offset_t*)ref->d_offs, (const mhip_offset_t*)reads->d_offs, d_cnt, d_ord);
    *d_order = d_ord;
    return 0;
}
