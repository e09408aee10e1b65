// cns_replay_m4_check.cpp — TEST INFRASTRUCTURE (tests/test_cns_cli_cpu.py builds it into a temporary directory): the m4 rule set of
// mecat_amd/csrc/cns_replay.h — cns_replay_m4_order and cns_replay_template_m4, the functions the accept stage runs on host threads —
// over a file of cases, plain g++ and no GPU.
// Input, int32 words: the number of cases; per case max_added, check_ratio, the ratio (a double as two words), n, and per record the
// overlap's qoff, qend, soff, send (what the order looks at), qsize, ssize, and the result of its alignment: ok, qoff, qend, soff, send.
// Output, a line per case: the number of records that become jobs, ':', then the accepted records as their numbers in the input, in
// acceptance order; '|'; then every record's number in the order the walk left the array in.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "cns_replay.h"

static FILE* g_in;
static int rd() {
    int v = 0;
    if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "short file\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2 || !(g_in = fopen(argv[1], "rb"))) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    const int ncases = rd();
    for (int c = 0; c < ncases; ++c) {
        CnsReplayM4Rules rules;
        rules.max_added = rd();
        rules.check_ratio = rd() != 0;
        int w[2] = {rd(), 0};
        w[1] = rd();
        memcpy(&rules.ratio, w, 8);
        const int n = rd();
        std::vector<mhip_ext_candidate> cands((size_t)n);
        std::vector<mhip_cns_result> by_tag((size_t)n);
        for (int i = 0; i < n; ++i) {
            mhip_ext_candidate& e = cands[(size_t)i];
            memset(&e, 0, sizeof(e));
            e.qoff = rd(); e.qend = rd(); e.soff = rd(); e.send = rd(); e.qsize = rd(); e.ssize = rd();
            e.score = i;                                  // the record's number: it travels with the record
            mhip_cns_result& r = by_tag[(size_t)i];
            memset(&r, 0, sizeof(r));
            r.ok = rd(); r.qoff = rd(); r.qend = rd(); r.soff = rd(); r.send = rd();
        }
        const int64_t njobs = cns_replay_m4_order(cands.data(), n, rules);
        std::vector<mhip_cns_result> res((size_t)njobs);          // job i is record i of the ordered array
        for (int64_t i = 0; i < njobs; ++i) res[(size_t)i] = by_tag[(size_t)cands[(size_t)i].score];
        const int64_t tmpl_begin[2] = {0, n}, jfirst[2] = {0, njobs};
        const std::vector<int32_t> acc = cns_replay_template_m4(cands.data(), tmpl_begin, res.data(), jfirst, 0, rules);
        printf("%lld:", (long long)njobs);
        for (const int32_t ji : acc) printf(" %d", cands[(size_t)ji].score);
        printf(" |");
        for (int i = 0; i < n; ++i) printf(" %d", cands[(size_t)i].score);
        printf("\n");
    }
    return 0;
}
