// aln_jobs_check.cpp — aln_jobs_check (mecat_amd/csrc/aln_jobs.h: the job check of mhip_align_candidates and mhip_xalign_candidates)
// on two reads of 20 and 30 bases, one case per rule: a stand-alone program, no GPU (test_aln_jobs_cpu.py builds and runs it).
// Prints every verdict; exit 0 when all are as expected.
#include "aln_jobs.h"

#include <string.h>

namespace {

const mhip_offset_t OFFS[2] = {{0, 20}, {21, 30}};      // both tables: read 0 has 20 bases, read 1 has 30
const int NUM_READS = 2;
const char* const RANGE = "alignment job %d: read index out of range";
const char* const START = "alignment job %d: start point outside the reads";

mhip_aln_job job(int qid, int sid, int qstart, int sstart) {
    mhip_aln_job j;
    memset(&j, 0, sizeof(j));
    j.qid_local = qid; j.sid_local = sid; j.qstart = qstart; j.sstart = sstart;
    return j;
}

int failures = 0;

// `j` between two valid jobs, at each of the three places of the list: accepted (why == NULL), or refused at its own index with `why`
void expect(const char* what, const mhip_aln_job& j, const char* why) {
    for (int at = 0; at < 3; ++at) {
        mhip_aln_job list[3] = {job(0, 1, 5, 7), job(1, 0, 30, 20), job(1, 1, 0, 0)};
        list[at] = j;
        char msg[96] = "";
        const int bad = aln_jobs_check(list, 3, OFFS, NUM_READS, OFFS, NUM_READS, msg, sizeof(msg));
        char want[96] = "";
        if (why) snprintf(want, sizeof(want), why, at);
        const bool ok = why ? (bad == at && strcmp(msg, want) == 0) : (bad == -1 && msg[0] == 0);
        printf("%-28s at %d: %s%s%s\n", what, at, bad < 0 ? "accepted" : "refused: ", msg, ok ? "" : "   <-- WRONG");
        failures += !ok;
    }
}

}  // namespace

int main() {
    expect("a valid job", job(0, 1, 10, 12), nullptr);
    expect("qstart < 0", job(0, 1, -1, 12), nullptr);      // a job without extension
    expect("qstart == size", job(0, 1, 20, 12), nullptr);
    expect("qstart == size + 1", job(0, 1, 21, 12), START);
    expect("sstart == size + 1", job(0, 1, 10, 31), START);
    expect("qid_local == -1", job(-1, 1, 10, 12), RANGE);
    expect("qid_local == num_reads", job(2, 1, 10, 12), RANGE);
    expect("sid_local == num_reads", job(0, 2, 10, 12), RANGE);
    // an empty list and a first failure in front of a second one
    char msg[96] = "";
    const mhip_aln_job two[2] = {job(0, 0, 21, 0), job(5, 0, 0, 0)};
    const bool ok = aln_jobs_check(two, 0, OFFS, NUM_READS, OFFS, NUM_READS, msg, sizeof(msg)) == -1 &&
                    aln_jobs_check(two, 2, OFFS, NUM_READS, OFFS, NUM_READS, msg, sizeof(msg)) == 0 && strcmp(msg, "alignment job 0: start point outside the reads") == 0;
    printf("%-28s      : %s\n", "empty list, first of two", ok ? "as expected" : "WRONG");
    failures += !ok;
    printf("aln_jobs_check: %d wrong\n", failures);
    return failures ? 1 : 0;
}
