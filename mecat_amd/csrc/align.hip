// align.hip — the dw extension's entry points: the job list from the candidate table, the two
// launches of the aligner, the stitch of the two directions.
//
// Two launches per call.  dw_extend2 (dw_extend2.hip) runs every (candidate, direction) unit, two per wave, and hands over the few it
// cannot finish; dw_extend (dw_extend.hip: one unit per wave, every row kept) finishes those from where they stand.  The second launch
// reads the number of handed-over units on the device, so nothing waits for the host in between.  dw_stitch then turns the two
// DirResults of a job into its mhip_aln_result.  MECAT_DW_KERNEL=1 (debug knob) runs every unit through dw_extend alone.
#include <stdlib.h>

#include "aln_jobs.h"
#include "dw_defs.h"
#include "scan.h"

// stitch the two directions (diff_gapalign.cpp:309-348)
__global__ void dw_stitch(const mhip_aln_job* __restrict__ jobs, const DirResult* __restrict__ dres, int n, int min_aln,
                          mhip_aln_result* __restrict__ out, unsigned long long* __restrict__ counters) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DirResult L = dres[2 * i], R = dres[2 * i + 1];
    mhip_aln_result r;
    r.query_start = jobs[i].qstart - L.qbases;
    r.target_start = jobs[i].sstart - L.tbases;
    r.query_end = jobs[i].qstart + R.qbases;
    r.target_end = jobs[i].sstart + R.tbases;
    r.matches = L.matches + R.matches;
    r.columns = L.columns + R.columns;
    r.blocks = L.blocks + R.blocks;
    r.ok = r.columns >= min_aln;
    out[i] = r;
    if (r.ok) {
        atomicAdd(&counters[6], (unsigned long long)(r.query_end - r.query_start));
        atomicAdd(&counters[7], 1ull);
    }
}

// candidate table -> job list (pw_impl.cpp:674-686): exclusive scan of the per-read counts (one block, running carry
// over 1024-read tiles), then one thread per (read, slot).
__global__ __launch_bounds__(1024) void dw_job_scan(const int32_t* __restrict__ counts, int n_reads, int part_index, int part_count,
                                                    unsigned int* __restrict__ first, int* __restrict__ num_jobs) {
    const unsigned int tot = scan_array_1024<unsigned int>(      // first[i]: global index of read i's first candidate
        n_reads, 0u, [&](long long i) { return (unsigned int)counts[i]; }, [&](long long i, unsigned int p) { first[i] = p; });
    if (threadIdx.x == 0) {
        unsigned int mine = tot;
        if (part_count > 1) mine = tot / (unsigned)part_count + ((unsigned)part_index < tot % (unsigned)part_count ? 1u : 0u);
        *num_jobs = (int)mine;
    }
}

__global__ __launch_bounds__(256) void dw_make_jobs(const mhip_candidate* __restrict__ cands, const int32_t* __restrict__ counts,
                                                    const unsigned int* __restrict__ first, int n_reads, int maxc, int rid_begin,
                                                    int rid_stride, int ref_start_id, int part_index, int part_count,
                                                    mhip_aln_job* __restrict__ jobs) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / (unsigned)maxc), j = (int)(t % (unsigned)maxc);
    if (i >= n_reads || j >= counts[i]) return;
    const unsigned int g = first[i] + (unsigned)j;
    if (part_count > 1 && (int)(g % (unsigned)part_count) != part_index) return;
    const unsigned int slot = part_count > 1 ? g / (unsigned)part_count : g;
    const mhip_candidate cd = cands[(size_t)i * maxc + j];
    mhip_aln_job jb;
    jb.qid_local = rid_begin + i * rid_stride;
    jb.sid_local = cd.readno - ref_start_id;
    jb.chain = cd.chain;
    int qstart = cd.loc2, sstart = cd.loc1;
    if (qstart && sstart) { qstart += MHIP_KMER_SIZE / 2; sstart += MHIP_KMER_SIZE / 2; }
    jb.qstart = qstart;
    jb.sstart = sstart;
    jobs[slot] = jb;
}

int aln_jobs_run(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const mhip_aln_job* jobs, int n, int min_align_size,
                 mhip_aln_result* out, aln_dev_fn dev) {
    HIPCHK(hipSetDevice(c->device));
    if (n <= 0) return 0;
    char why[96];
    if (aln_jobs_check(jobs, n, reads->h_offs.data(), reads->num_reads, ref->h_offs.data(), ref->num_reads, why, sizeof(why)) >= 0) {
        mhip_set_error("%s", why);
        return -1;
    }
    mhip_aln_job* d_jobs;
    mhip_aln_result* d_out;
    if (c->scratch("al_jobs", sizeof(mhip_aln_job) * (size_t)n, (void**)&d_jobs)) return -1;
    if (c->scratch("al_out", sizeof(mhip_aln_result) * (size_t)n, (void**)&d_out)) return -1;
    HIPCHK(hipMemcpyAsync(d_jobs, jobs, sizeof(mhip_aln_job) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (dev(c, ref, reads, d_jobs, n, min_align_size, d_out)) return -1;
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(mhip_aln_result) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" {

int mhip_jobs_from_candidates_dev(mhip_ctx* c, const void* d_cands, const void* d_counts, int n_reads, int maxc, int rid_begin,
                                  int rid_stride, int ref_start_read_id, int part_index, int part_count, void* d_jobs, int* num_jobs) {
    HIPCHK(hipSetDevice(c->device));
    *num_jobs = 0;
    if (n_reads <= 0) return 0;
    if (part_count < 1) part_count = 1;
    int* d_n;
    if (c->scratch("al_njobs", 64, (void**)&d_n)) return -1;
    unsigned int* d_first;
    if (c->scratch("al_jobfirst", sizeof(unsigned int) * (size_t)n_reads, (void**)&d_first)) return -1;
    LAUNCH(c, "dw_job_scan", dw_job_scan, 1, 1024, 0, (const int32_t*)d_counts, n_reads, part_index, part_count, d_first, d_n);
    const size_t nthreads = (size_t)n_reads * (size_t)maxc;
    LAUNCH(c, "dw_make_jobs", dw_make_jobs, (unsigned)((nthreads + 255) / 256), 256, 0, (const mhip_candidate*)d_cands,
           (const int32_t*)d_counts, (const unsigned int*)d_first, n_reads, maxc, rid_begin, rid_stride, ref_start_read_id, part_index,
           part_count, (mhip_aln_job*)d_jobs);
    HIPCHK(hipMemcpyAsync(num_jobs, d_n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int mhip_align_candidates_dev(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n,
                              int min_align_size, void* d_out) {
    HIPCHK(hipSetDevice(c->device));
    if (n <= 0) return 0;
    DirResult* d_dres;
    unsigned int* d_cur;      // the 16-byte cursor block: [0] unit cursor of the first launch, [1] units handed over, [2] cursor of the second launch
    if (c->scratch("al_dres", sizeof(DirResult) * 2 * (size_t)n, (void**)&d_dres)) return -1;
    if (c->scratch("al_cursor", 64, (void**)&d_cur)) return -1;
    HIPCHK(hipMemsetAsync(d_cur, 0, 16, c->stream));
    const char* kv = getenv("MECAT_DW_KERNEL");      // debug knob: 1 = one unit per wave, default 2 = one unit per half-wave
    if (kv && atoi(kv) == 1) {
        if (dw_extend_launch(c, ref, reads, d_jobs, n, d_dres, nullptr, nullptr, d_cur)) return -1;
    } else {
        DwHandover* d_hand;
        if (c->scratch("al_hand", sizeof(DwHandover) * 2 * (size_t)n, (void**)&d_hand)) return -1;
        if (dw_extend2_launch(c, ref, reads, d_jobs, n, d_dres, d_hand, d_cur + 1, d_cur)) return -1;
        // the units it handed over (a fraction of a percent); the launch reads their number on the device
        if (dw_extend_launch(c, ref, reads, d_jobs, n, d_dres, d_hand, d_cur + 1, d_cur + 2)) return -1;
    }
    LAUNCH(c, "dw_stitch", dw_stitch, (n + 255) / 256, 256, 0, (const mhip_aln_job*)d_jobs, (const DirResult*)d_dres, n,
           min_align_size, (mhip_aln_result*)d_out, (unsigned long long*)c->d_counters);
    HIPCHK(hipGetLastError());
    return 0;
}

int mhip_align_candidates(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const mhip_aln_job* jobs, int n,
                          int min_align_size, mhip_aln_result* out) {
    return aln_jobs_run(c, ref, reads, jobs, n, min_align_size, out, mhip_align_candidates_dev);
}

}  // extern "C"
