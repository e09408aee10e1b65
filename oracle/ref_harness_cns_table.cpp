// ref_harness_cns_table.cpp — TEST INFRASTRUCTURE: exposes the consensus table of the UNMODIFIED mecat2cns (see oracle/Makefile target
// `ref`).  src/mecat2cns/mecat_correction.cpp is compiled as part of THIS translation unit, included where it lies, because
// identify_one_consensus_item (:14-24) is `inline` there and has no symbol of its own; the rest of mecat2cns is linked as usual, minus
// that one file.  Three things come out:
//   refc_consensus_can_table   consensus_one_read_can_pacbio / _nanopore on one template, as refa_consensus_can of
//                              ref_harness_cns_accept.cpp runs it, plus the read_size CnsTableItems that the call left in
//                              ConsensusThreadData::cns_table (consensus_worker only reads them, :203-239)
//   refc_add_one_aln           meap_add_one_aln (:36-60) on a caller-owned table
//   refc_identify              identify_one_consensus_item on one item
// Pins mhip_cns_accept_templates_ex's table and mhip_debug_cns_table (tests/golden/make_golden_cns_table.py); never linked by the
// product path.
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "mecat2cns/mecat_correction.cpp"

using namespace ns_meap_cns;

static PackedDB* g_reads = NULL;
static ConsensusThreadData* g_ctd = NULL;
static std::ostringstream g_sink;

extern "C" {

int refc_item_size(void) { return (int)sizeof(CnsTableItem); }

// all reads from a FASTA file, as mecat2cns loads them (reads_correction_can.cpp)
int refc_load_reads(const char* fasta) {
    delete g_reads;
    g_reads = new PackedDB();
    g_reads->load_fasta_db(fasta);
    return (int)g_reads->num_seqs();
}

// candidates: n x 13 ints in ExtensionCandidate field order, all of ONE template (sid == read_id); sorted in place by the reference.
// Returns the number of accepted alignments; out_meta[4 * i ..] = {soff, send, aln_size, -1}, strings appended to out_strings as
// qaln NUL saln NUL (both as refa_consensus_can); out_table = the template's read_size items as the reference left them, *out_read_size
// their number.  -1: out_strings too small, -2: out_table too small.
int refc_consensus_can_table(int tech, int* cands, int n, int read_id, int min_align_size, double min_mapping_ratio, int* out_meta,
                             char* out_strings, long out_cap, long* out_used, void* out_table, int table_cap, int* out_read_size) {
    if (n <= 0) return -3;
    ReadsCorrectionOptions rco;
    memset(&rco, 0, sizeof(rco));
    rco.input_type = INPUT_TYPE_CAN;
    rco.num_threads = 1;
    rco.min_mapping_ratio = min_mapping_ratio;
    rco.min_align_size = min_align_size;
    rco.min_cov = tech == TECH_PACBIO ? 4 : 6;         // mecat2cns defaults (options.cpp); they only steer consensus_worker
    rco.min_size = tech == TECH_PACBIO ? 5000 : 2000;
    rco.tech = tech;
    delete g_ctd;
    g_ctd = new ConsensusThreadData(&rco, 0, g_reads, (ExtensionCandidate*)cands, n, &g_sink);
    const int read_size = ((ExtensionCandidate*)cands)[0].ssize;      // what consensus_one_read_can_* clears and fills (:398, :414)
    if (read_size > table_cap) return -2;
    if (tech == TECH_PACBIO) consensus_one_read_can_pacbio(g_ctd, read_id, 0, n);
    else consensus_one_read_can_nanopore(g_ctd, read_id, 0, n);
    long used = 0;
    int k = 0;
    for (CnsAln* a = g_ctd->cns_alns.begin(); a != g_ctd->cns_alns.end(); ++a, ++k) {
        int tb = 0;                                    // consensus_worker advances CnsAln::soff: re-derived from send
        for (int i = 0; i < a->aln_size; ++i) tb += a->saln[i] != '-';
        out_meta[4 * k] = a->send - tb;
        out_meta[4 * k + 1] = a->send;
        out_meta[4 * k + 2] = a->aln_size;
        out_meta[4 * k + 3] = -1;
        if (used + 2L * (a->aln_size + 1) > out_cap) return -1;
        memcpy(out_strings + used, a->qaln, (size_t)a->aln_size + 1);
        used += a->aln_size + 1;
        memcpy(out_strings + used, a->saln, (size_t)a->aln_size + 1);
        used += a->aln_size + 1;
    }
    *out_used = used;
    memcpy(out_table, g_ctd->cns_table, sizeof(CnsTableItem) * (size_t)read_size);
    *out_read_size = read_size;
    g_ctd->cns_results.clear();
    return k;
}

// meap_add_one_aln(q, s, soff, table) on `table` (tmpl_len items, read and written: calls add up).  The reference sees the table one
// item into a buffer of tmpl_len + 2 items whose first and last are fresh guard items, returned in guards[0] / guards[1]: a run of
// template gaps in front of the first template base at soff == 0 makes the reference count at index -1, which is the front guard here.
// Refused before the reference is called (it would abort or overrun): -1 a column with two different bases, -2 a template span
// outside [0, tmpl_len).
int refc_add_one_aln(const char* q, const char* s, int n, int soff, void* table, int tmpl_len, void* guards) {
    if (n < 0 || tmpl_len < 0) return -2;
    long span = 0;
    for (int i = 0; i < n; ++i) {
        if (q[i] != '-' && s[i] != '-' && q[i] != s[i]) return -1;
        span += s[i] != '-';
    }
    if (soff < 0 || soff + span > tmpl_len) return -2;
    std::vector<CnsTableItem> buf((size_t)tmpl_len + 2);      // (CnsTableItem(): 'N', 0, 0, 0)
    if (tmpl_len) memcpy(&buf[1], table, sizeof(CnsTableItem) * (size_t)tmpl_len);
    const std::string qs(q, (size_t)n), ss(s, (size_t)n);
    meap_add_one_aln(qs, ss, soff, &buf[1], NULL);
    if (tmpl_len) memcpy(table, &buf[1], sizeof(CnsTableItem) * (size_t)tmpl_len);
    memcpy(guards, &buf[0], sizeof(CnsTableItem));
    memcpy((char*)guards + sizeof(CnsTableItem), &buf[(size_t)tmpl_len + 1], sizeof(CnsTableItem));
    return 0;
}

// identify_one_consensus_item on {mat, ins, del} (min_cov is not read by it)
int refc_identify(int mat, int ins, int del) {
    CnsTableItem it;
    it.mat_cnt = (uint1)mat;
    it.ins_cnt = (uint1)ins;
    it.del_cnt = (uint1)del;
    return identify_one_consensus_item(it, 0);
}

// the same over n items of a table (4 bytes each)
void refc_identify_table(const void* table, int n, unsigned char* ident) {
    for (int i = 0; i < n; ++i) {
        CnsTableItem it;
        memcpy(&it, (const char*)table + sizeof(CnsTableItem) * (size_t)i, sizeof(CnsTableItem));
        ident[i] = identify_one_consensus_item(it, 0);
    }
}

// the same over n triples {mat, ins, del} of ints
void refc_identify_triples(const int* mid, long n, unsigned char* ident) {
    for (long i = 0; i < n; ++i) ident[i] = (unsigned char)refc_identify(mid[3 * i], mid[3 * i + 1], mid[3 * i + 2]);
}

}  // extern "C"
