// cns_cli_ref_main.cpp — TEST INFRASTRUCTURE (tests/golden/make_golden_cns_cli.py builds it into a temporary directory; the binary is
// never committed): a main in front of the UNMODIFIED mecat2cns, compiled against the reference's headers where they lie and linked with
// oracle/_ref/libref_cns_accept.so, which holds all of mecat2cns except main.cpp.
//   cns_cli_ref_main cli <argv of mecat2cns ...>
//       parse_arguments, print_options, print_usage and reads_correction_can / reads_correction_m4 in the order of the reference's main:
//       the reference program under another name (argv[0] of the recorded usage text is "mecat2cns").
//   cns_cli_ref_main m4walk <partition file> <reads.fasta> <tech> <min_align_size> <min_mapping_ratio> <min_cov> <min_size> <out.bin>
//       the m4 walk over one partition file the way reads_correction_m4.cpp drives it with one thread: build_cns_thrd_data_can (the
//       whole-array sort by sid), the two gates, consensus_one_read_m4_*.  Per template that passes the gates the file gets: int32 sid,
//       number of records, records the walk looks at, how many of those GetAlignment accepts (our own second call per record, on the
//       array as the walk left it) and how many of the accepted the mapping-range check refuses (nanopore's rule, counted for both);
//       per record looked at int32 ok, qoff, qend, soff, send (of that second call; zeros where it failed), qsize, ssize;
//       int32 number of cns_alns entries, per entry soff, send, aln_size and the two strings with their NULs; int32 number of
//       cns_results, per result id, range[0], range[1], size and the letters.  At the end int32 -1 and the two gates' drop counts.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <vector>

#include "mecat2cns/mecat_correction.h"
#include "mecat2cns/overlaps_store.h"
#include "mecat2cns/reads_correction_aux.h"
#include "mecat2cns/reads_correction_can.h"
#include "mecat2cns/reads_correction_m4.h"

static void put(FILE* f, int v) { fwrite(&v, 4, 1, f); }

static int run_cli(int argc, char** argv) {
    ReadsCorrectionOptions rco;
    memset(&rco, 0, sizeof(rco));      // (the reference prints the struct even where parse_arguments returned before filling it)
    const int r = parse_arguments(argc, argv, rco);
    print_options(rco);
    fflush(stdout);
    if (r) { print_usage(argv[0]); return 1; }
    if (rco.print_usage_info) { print_usage(argv[0]); return 0; }
    return rco.input_type == INPUT_TYPE_CAN ? reads_correction_can(rco) : reads_correction_m4(rco);
}

static int run_m4walk(char** a) {
    ReadsCorrectionOptions rco;
    memset(&rco, 0, sizeof(rco));
    rco.input_type = INPUT_TYPE_M4;
    rco.num_threads = 1;
    rco.tech = atoi(a[2]);
    rco.min_align_size = atoi(a[3]);
    rco.min_mapping_ratio = atof(a[4]);
    rco.min_cov = atoi(a[5]);
    rco.min_size = atoi(a[6]);
    FILE* out = fopen(a[7], "wb");
    if (!out) { perror(a[7]); return 2; }
    PackedDB reads;
    reads.load_fasta_db(a[1]);
    idx_t nec = 0;
    ExtensionCandidate* ec = load_partition_data<ExtensionCandidate>(a[0], nec);
    if (nec == 0) { put(out, -1); put(out, 0); put(out, 0); fclose(out); return 0; }
    idx_t lo = ec[0].sid, hi = ec[0].sid;
    for (idx_t i = 0; i < nec; ++i) { lo = std::min<idx_t>(lo, ec[i].sid); hi = std::max<idx_t>(hi, ec[i].sid); }
    std::ostringstream sink;
    ConsensusThreadData* pctd[1] = {NULL};
    build_cns_thrd_data_can(ec, (int)nec, lo, hi + 1, &rco, &reads, &sink, pctd);
    ConsensusThreadData& ctd = *pctd[0];
    if (ctd.num_candidates != nec) { fprintf(stderr, "the one thread did not get the whole array\n"); return 2; }
    const int max_added = rco.tech == TECH_PACBIO ? 60 : MAX_CNS_OVLPS;
    const double error_rate = rco.tech == TECH_PACBIO ? 0.15 : 0.20, ratio = rco.min_mapping_ratio - 0.02;
    int drop_cov = 0, drop_size = 0;
    std::vector<char> q, t;
    for (idx_t i = 0, j; i < nec; i = j) {
        const idx_t sid = ec[i].sid;
        j = i + 1;
        while (j < nec && ec[j].sid == sid) ++j;
        if (j - i < rco.min_cov) { ++drop_cov; continue; }
        if (ec[i].ssize < rco.min_size * 0.95) { ++drop_size; continue; }
        ctd.cns_results.clear();
        if (rco.tech == TECH_PACBIO) ns_meap_cns::consensus_one_read_m4_pacbio(&ctd, sid, i, j);
        else ns_meap_cns::consensus_one_read_m4_nanopore(&ctd, sid, i, j);
        // what the walk saw, counted again on the array as it left it
        const int looked = (int)std::min<idx_t>(j - i, max_added);
        int aligned = 0, ratio_refused = 0;
        std::vector<int> seen;
        t.resize(ec[i].ssize);
        reads.GetSequence(sid, true, t.data(), ec[i].ssize);
        for (idx_t k = i; k < i + looked; ++k) {
            const ExtensionCandidate& o = ec[k];
            q.resize(o.qsize);
            reads.GetSequence(o.qid, o.qdir == FWD, q.data(), o.qsize);
            const int qext = o.qdir == REV ? o.qsize - 1 - o.qext : o.qext;
            M5Record& m5 = *ctd.m5;
            const bool ok = ns_banded_sw::GetAlignment(q.data(), qext, o.qsize, t.data(), o.sext, o.ssize, ctd.drd_s, m5, error_rate, rco.min_align_size);
            const int row[7] = {ok, ok ? (int)m5qoff(m5) : 0, ok ? (int)m5qend(m5) : 0, ok ? (int)m5soff(m5) : 0, ok ? (int)m5send(m5) : 0, (int)o.qsize, (int)o.ssize};
            seen.insert(seen.end(), row, row + 7);
            if (!ok) continue;
            ++aligned;
            const int oq = m5qend(m5) - m5qoff(m5), qqs = o.qsize * ratio, os = m5send(m5) - m5soff(m5), qss = o.ssize * ratio;
            ratio_refused += !(oq >= qqs || os >= qss);
        }
        put(out, (int)sid); put(out, (int)(j - i)); put(out, looked); put(out, aligned); put(out, ratio_refused);
        fwrite(seen.data(), 4, seen.size(), out);
        put(out, (int)ctd.cns_alns.num_alns());
        for (CnsAln* x = ctd.cns_alns.begin(); x != ctd.cns_alns.end(); ++x) {
            int tb = 0;      // (consensus_worker advances soff while it reads the alignments: re-derived from the string)
            for (int c = 0; c < x->aln_size; ++c) tb += x->saln[c] != '-';
            put(out, x->send - tb); put(out, x->send); put(out, x->aln_size);
            fwrite(x->qaln, 1, (size_t)x->aln_size + 1, out);
            fwrite(x->saln, 1, (size_t)x->aln_size + 1, out);
        }
        put(out, (int)ctd.cns_results.size());
        for (const CnsResult& r : ctd.cns_results) {
            put(out, (int)r.id); put(out, (int)r.range[0]); put(out, (int)r.range[1]); put(out, (int)r.seq.size());
            fwrite(r.seq.data(), 1, r.seq.size(), out);
        }
    }
    put(out, -1); put(out, drop_cov); put(out, drop_size);
    fclose(out);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "cli") == 0) {
        argv[1] = (char*)"mecat2cns";
        return run_cli(argc - 1, argv + 1);
    }
    if (argc == 10 && strcmp(argv[1], "m4walk") == 0) return run_m4walk(argv + 2);
    fprintf(stderr, "usage: %s cli <mecat2cns arguments> | m4walk <partition> <reads> <tech> <min_align_size> <ratio> <min_cov> <min_size> <out>\n", argv[0]);
    return 2;
}
