// aln_jobs.h — the host side both pairwise aligners share (align.hip: dw; xalign.hip: X-drop): the check of a job list that comes from
// the host, and the upload / run / download around an aligner's _dev entry point.  Host only, no HIP in it.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "mecat_hip.h"

// Checks jobs [0, n) against the offset tables of the query reads (q_offs, q_reads of them) and of the subject reads.  Two rules: both
// read indices inside their table; neither start point behind the end of its read (a start point at the end is an extension of
// nothing; a negative one is a job without extension, see dw_extend).  Returns -1 when all pass; otherwise the index of the first
// job that fails, with the reason in msg.
inline int aln_jobs_check(const mhip_aln_job* jobs, int n, const mhip_offset_t* q_offs, int q_reads, const mhip_offset_t* s_offs, int s_reads,
                          char* msg, size_t msg_cap) {
    for (int i = 0; i < n; ++i) {
        const mhip_aln_job& j = jobs[i];
        if (j.qid_local < 0 || j.qid_local >= q_reads || j.sid_local < 0 || j.sid_local >= s_reads) {
            snprintf(msg, msg_cap, "alignment job %d: read index out of range", i);
            return i;
        }
        if (j.qstart > q_offs[(size_t)j.qid_local].size || j.sstart > s_offs[(size_t)j.sid_local].size) {
            snprintf(msg, msg_cap, "alignment job %d: start point outside the reads", i);
            return i;
        }
    }
    return -1;
}

// an aligner over device-resident jobs: mhip_align_candidates_dev, mhip_xalign_candidates_dev
typedef int (*aln_dev_fn)(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n, int min_align_size, void* d_out);

// align.hip: checks the jobs, uploads them (scratch "al_jobs"), runs `dev`, downloads the results (scratch "al_out") and waits
int aln_jobs_run(mhip_ctx* c, const mhip_volume* ref, const mhip_volume* reads, const mhip_aln_job* jobs, int n, int min_align_size,
                 mhip_aln_result* out, aln_dev_fn dev);
