// cns_poa_ref_main.cpp — TEST INFRASTRUCTURE (tests/golden/make_golden_cns_poa.py builds it into a temporary directory; the binary is
// never committed): the UNMODIFIED meap_cns_one_indel (mecat2cns/mecat_correction.cpp:62-78) over a file of packed cases.  Compiled
// against the reference's headers where they lie and linked with oracle/_ref/libref_cns_table.so, which exports the function.  Per case
// (one template) it fills a CnsAlns with add_aln and calls meap_cns_one_indel for the case's windows in order, the reference's own
// cursors included; a case flagged `fresh` gets a newly filled CnsAlns in front of every window.  Input: tests/cns_poa_cases.py
// write_cases (the pieces and recorded strings a file may hold behind a case's windows are skipped).  Output: per window an int32
// length and the bytes of `cns`.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "mecat2cns/reads_correction_aux.h"

namespace ns_meap_cns {
void meap_cns_one_indel(const int sb, const int se, CnsAlns& cns_vec, const int min_cov, std::string& aux_qstr, std::string& aux_tstr, std::string& cns);
}

static FILE* g_in;
static int rd() {
    int v = 0;
    if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "short file\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    g_in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!g_in || !out) { perror("open"); return 2; }
    if (rd() != 0x504f4131) { fprintf(stderr, "not a case file\n"); return 2; }
    const int ncases = rd();
    const int has_tail = rd();
    CnsAlns* alns = new CnsAlns();
    std::string aq, at, cns;
    for (int c = 0; c < ncases; ++c) {
        const int fresh = rd(), na = rd();
        std::vector<int> soff(na), send(na);
        std::vector<std::string> q(na), s(na);
        for (int a = 0; a < na; ++a) {
            soff[a] = rd(); send[a] = rd();
            const int n = rd();
            q[a].resize(n); s[a].resize(n);
            if (n && (fread(&q[a][0], 1, n, g_in) != (size_t)n || fread(&s[a][0], 1, n, g_in) != (size_t)n)) { fprintf(stderr, "short file\n"); return 2; }
        }
        const int nw = rd();
        std::vector<int> win(3 * (size_t)nw);
        for (size_t i = 0; i < win.size(); ++i) win[i] = rd();
        if (has_tail) {
            std::vector<int> pb(nw + 1);
            for (int w = 0; w <= nw; ++w) pb[w] = rd();
            for (int i = 0; i < 4 * pb[nw]; ++i) rd();
            for (int w = 0; w < nw; ++w) {
                const int n = rd();
                if (fseek(g_in, n, SEEK_CUR)) return 2;
            }
        }
        for (int w = 0; w < nw; ++w) {
            if (w == 0 || fresh) {
                alns->clear();
                for (int a = 0; a < na; ++a) alns->add_aln(soff[a], send[a], q[a], s[a]);
            }
            ns_meap_cns::meap_cns_one_indel(win[3 * w], win[3 * w + 1], *alns, win[3 * w + 2], aq, at, cns);
            const int n = (int)cns.size();
            fwrite(&n, 4, 1, out);
            fwrite(cns.data(), 1, cns.size(), out);
        }
    }
    fclose(out);
    return 0;
}
