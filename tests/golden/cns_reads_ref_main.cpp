// cns_reads_ref_main.cpp — TEST INFRASTRUCTURE (tests/golden/make_golden_cns_reads.py builds it into a temporary directory; the binary is
// never committed): the UNMODIFIED back end of mecat2cns behind the accept loop — meap_add_one_aln, CnsAlns::add_aln,
// get_effective_ranges and consensus_worker (mecat2cns/mecat_correction.cpp:36-60, :118-153, :203-239) — over a file of packed cases.
// Compiled against the reference's headers where they lie and linked with oracle/_ref/libref_cns_table.so, which holds
// mecat_correction.cpp whole and exports these functions.  Per case (one template) it clears a table as consensus_one_read_can_* does
// (:414), adds every alignment to the table and to the CnsAlns (:439-440), takes the effective ranges (tech 0: :445-447; tech 1: the
// whole read, :509), calls consensus_worker (:449) and writes the cns_results it pushed.  Input: tests/cns_reads_ref.py write_cases.
// Output: per case an int32 count, per result int32 id, range[0], range[1], size and the bytes of seq.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mecat2cns/reads_correction_aux.h"

namespace ns_meap_cns {
void meap_add_one_aln(const std::string& qaln, const std::string& saln, index_t start_soff, CnsTableItem* cns_table, const char* org_seq);
void get_effective_ranges(std::vector<MappingRange>& mranges, std::vector<MappingRange>& eranges, const int read_size, const int min_size);
void consensus_worker(CnsTableItem* cns_table, uint1* id_list, CnsAlns& cns_vec, std::string& aux_qstr, std::string& aux_tstr, std::vector<MappingRange>& eranges,
                      const int min_cov, const int min_size, const int read_id, std::vector<CnsResult>& cns_results);
}

static FILE* g_in;
static int rd() {
    int v = 0;
    if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "short file\n"); exit(2); }
    return v;
}
static void rd_bytes(std::string& s, int n) {
    s.resize((size_t)n);
    if (n && fread(&s[0], 1, (size_t)n, g_in) != (size_t)n) { fprintf(stderr, "short file\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    g_in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!g_in || !out) { perror("open"); return 2; }
    if (rd() != 0x52454131) { fprintf(stderr, "not a case file\n"); return 2; }
    const int ncases = rd();
    CnsAlns* alns = new CnsAlns();
    std::vector<CnsTableItem> table;
    std::vector<uint1> id_list;
    std::string aq, at, q, s, tmpl;
    for (int c = 0; c < ncases; ++c) {
        const int tech = rd(), min_cov = rd(), min_size = rd(), read_id = rd(), L = rd();
        rd_bytes(tmpl, L);
        if (L >= MAX_SEQ_SIZE) { fprintf(stderr, "case %d: template too long\n", c); return 2; }
        table.resize((size_t)L + 1);
        id_list.assign((size_t)L + 1, 0);
        std::for_each(table.begin(), table.end(), CnsTableItemCleaner());
        alns->clear();
        const int na = rd();
        if (na > MAX_CNS_OVLPS) { fprintf(stderr, "case %d: %d alignments\n", c, na); return 2; }
        for (int a = 0; a < na; ++a) {
            const int soff = rd(), send = rd(), n = rd();
            rd_bytes(q, n);
            rd_bytes(s, n);
            ns_meap_cns::meap_add_one_aln(q, s, soff, table.data(), tmpl.data());
            alns->add_aln(soff, send, q, s);
        }
        std::vector<MappingRange> mranges, eranges;
        if (tech == TECH_PACBIO) {
            alns->get_mapping_ranges(mranges);
            ns_meap_cns::get_effective_ranges(mranges, eranges, L, min_size);
        } else {
            eranges.push_back(MappingRange(0, L));
        }
        std::vector<CnsResult> results;
        ns_meap_cns::consensus_worker(table.data(), id_list.data(), *alns, aq, at, eranges, min_cov, min_size, read_id, results);
        const int nres = (int)results.size();
        fwrite(&nres, 4, 1, out);
        for (const CnsResult& r : results) {
            const int rec[4] = {(int)r.id, (int)r.range[0], (int)r.range[1], (int)r.seq.size()};
            fwrite(rec, 4, 4, out);
            fwrite(r.seq.data(), 1, r.seq.size(), out);
        }
    }
    fclose(out);
    return 0;
}
