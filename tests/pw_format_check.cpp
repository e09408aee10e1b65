// pw_format_check.cpp — format_can_read / format_m4_read (mecat_amd/host/pw_format.h: the functions the mecat2pw driver turns a read's
// candidates and extension results into lines with) on a case file: a stand-alone program for the sanitizers (test_pw_format_cpu.py
// writes the cases, builds this with -fsanitize=address,undefined and compares the lines, read by read, with the oracle's).
// usage: pw_format_check <case file> can|m4g0|m4g1     prints "== <read>" and the read's lines, for every read in order
#include "pw_format.h"

#include <stdio.h>
#include <string.h>

static int geti(FILE* f) {
    int v;
    if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "case file ends early\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    const bool can = !strcmp(argv[2], "can"), gapped = !strcmp(argv[2], "m4g1");
    const int nq = geti(f), q_start = geti(f), nref = geti(f), ref_start = geti(f);
    std::vector<mhip_offset_t> q_offs((size_t)nq), ref_offs((size_t)nref);
    int at = 0;
    for (mhip_offset_t& o : q_offs) { o.offset = at; o.size = geti(f); at += o.size + 1; }
    at = 0;
    for (mhip_offset_t& o : ref_offs) { o.offset = at; o.size = geti(f); at += o.size + 1; }
    const CellReads T = {q_offs.data(), q_start, ref_offs.data(), ref_start};
    M4Scratch scratch;
    for (int r = 0; r < nq; ++r) {
        const int n = geti(f);
        // exactly n entries each: a read past the end of either list is the sanitizer's to find
        std::vector<mhip_candidate> cands((size_t)n);
        std::vector<mhip_aln_result> res((size_t)n);
        for (int k = 0; k < n; ++k) {
            mhip_candidate& c = cands[(size_t)k];
            memset(&c, 0, sizeof(c));
            c.readno = geti(f); c.chain = geti(f); c.loc1 = geti(f); c.loc2 = geti(f); c.score = geti(f);
            mhip_aln_result& a = res[(size_t)k];
            a.ok = geti(f); a.query_start = geti(f); a.query_end = geti(f); a.target_start = geti(f); a.target_end = geti(f);
            a.matches = geti(f); a.columns = geti(f); a.blocks = 0;
        }
        std::string text;
        std::vector<CanRec> crec;
        std::vector<M4Rec> mrec;
        if (can) format_can_read(T, r, cands.data(), n, text, &crec);
        else format_m4_read(T, r, cands.data(), res.data(), n, gapped, scratch, text, &mrec);
        const size_t lines = (size_t)std::count(text.begin(), text.end(), '\n');
        if (lines != (can ? crec.size() : mrec.size())) { fprintf(stderr, "read %d: %zu lines, %zu records\n", r, lines, can ? crec.size() : mrec.size()); return 1; }
        printf("== %d\n%s", r, text.c_str());
    }
    fclose(f);
    return 0;
}
