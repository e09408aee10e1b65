// pw_format.h — what one query read becomes in the output: its `.can` lines (common/alignment.cpp:18-32) or its `.m4` lines after
// the per-read post-filter (std::sort + containment, pw_impl.cpp:539-610; line format :509-531).  No HIP call and no thread: plain
// functions over the read tables and the arrays the library returns.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mecat_hip.h"
#include "partition.h"

struct M4Record {      // common/alignment.h:21-37
    int64_t qid, sid;
    double ident;
    int vscore, qdir;
    int64_t qoff, qend, qsize;
    int sdir;
    int64_t soff, send, ssize, qext, sext;
};

struct CmpM4ByQidAndOvlpSize {   // pw_impl.cpp:539-548 ; std::sort keeps libstdc++'s tie order like the reference
    bool operator()(const M4Record& a, const M4Record& b) const {
        if (a.qid != b.qid) return a.qid < b.qid;
        const int64_t qa = a.qend - a.qoff, sa = a.send - a.soff, qb = b.qend - b.qoff, sb = b.send - b.soff;
        const int o1 = (int)std::min(qa, sa), o2 = (int)std::min(qb, sb);
        return o1 > o2;
    }
};

// pw_impl.cpp:550-574
static void check_records_containment(const M4Record* v, int s, int e, std::vector<int>& valid) {
    const int soft = 100;
    for (int i = s; i < e; ++i) {
        if (!valid[i]) continue;
        const int qb1 = (int)v[i].qoff, qe1 = (int)v[i].qend, sb1 = (int)v[i].soff, se1 = (int)v[i].send;
        for (int j = i + 1; j < e; ++j) {
            if (!valid[j]) continue;
            if (v[i].sdir != v[j].sdir) continue;
            const int qb2 = (int)v[j].qoff, qe2 = (int)v[j].qend, sb2 = (int)v[j].soff, se2 = (int)v[j].send;
            if (qb2 + soft >= qb1 && qe2 - soft <= qe1 && sb2 + soft >= sb1 && se2 - soft <= se1) valid[j] = 0;
        }
    }
}

// "%d" of printf, without printf: the digits of v at p, returns the position behind them
static inline char* put_int(char* p, int v) {
    unsigned int u = (unsigned int)v;
    if (v < 0) { *p++ = '-'; u = 0u - u; }
    char tmp[12];
    int n = 0;
    do { tmp[n++] = (char)('0' + u % 10u); u /= 10u; } while (u);
    while (n) *p++ = tmp[--n];
    return p;
}

// the read tables of a grid cell: query volume and reference volume (volume.h's HostVolume::offs / start_read_id)
struct CellReads {
    const mhip_offset_t* q_offs;
    int q_start_id;
    const mhip_offset_t* ref_offs;
    int ref_start_id;
};

// the extension job of a candidate of query read `q_local` (the loop head of pairwise_mapping, pw_impl.cpp:674-686): the subject's index
// in the reference volume and the start points, moved half a k-mer inwards unless one of them is 0.  (The device derives the same in
// mhip_jobs_from_candidates_dev; the text is made from these fields, not from what the device assembled.)
static inline mhip_aln_job job_of_candidate(const mhip_candidate& c, int q_local, int ref_start_id) {
    mhip_aln_job j;
    j.qid_local = q_local;
    j.sid_local = c.readno - ref_start_id;
    j.chain = c.chain;
    j.qstart = c.loc2;
    j.sstart = c.loc1;
    if (j.qstart && j.sstart) { j.qstart += MHIP_KMER_SIZE / 2; j.sstart += MHIP_KMER_SIZE / 2; }
    return j;
}

// candidate_detect, pw_impl.cpp:767-801: the `.can` lines of query read q_local's n candidates, appended to o (and, with recs, the same
// lines in the same order as records: SURVEY.md §8f row N4, no text round trip)
static inline void format_can_read(const CellReads& T, int q_local, const mhip_candidate* cands, int n, std::string& o, std::vector<CanRec>* recs) {
    const int qsize = T.q_offs[q_local].size, qid = q_local + T.q_start_id;
    char line[160];
    for (int k = 0; k < n; ++k) {
        const mhip_candidate& c = cands[k];
        const mhip_aln_job j = job_of_candidate(c, q_local, T.ref_start_id);
        int qext = j.qstart;
        const int sext = j.sstart, ssize = T.ref_offs[j.sid_local].size;
        if (c.chain == 1) qext = qsize - 1 - qext;
        // ("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n": nine integers a line, two million lines at config 2 — snprintf was most of the
        // drop-in's -j 0 wall time behind the device)
        char* p = line;
        const int f[9] = {qid, c.readno, c.chain, 0, qext, sext, c.score, qsize, ssize};
        for (int q = 0; q < 9; ++q) { p = put_int(p, f[q]); *p++ = q == 8 ? '\n' : '\t'; }
        o.append(line, (size_t)(p - line));
        if (recs) recs->push_back(CanRec{qid, c.readno, c.chain, 0, qext, sext, c.score, qsize, ssize});
    }
}

struct M4Scratch {      // per thread, reused from read to read
    std::vector<M4Record> m4v;
    std::vector<int> valid;
};

// the `.m4` lines of query read q_local: res[k] is the extension of cands[k]; records of the accepted ones (fill_m4record), the
// post-filter (append_m4v), the lines (with the gapped start points when `gapped`), appended to o and, with recs, as records
static inline void format_m4_read(const CellReads& T, int q_local, const mhip_candidate* cands, const mhip_aln_result* res, int n, bool gapped,
                                  M4Scratch& S, std::string& o, std::vector<M4Rec>* recs) {
    const int qsize = T.q_offs[q_local].size, qid = q_local + T.q_start_id;
    std::vector<M4Record>& m4v = S.m4v;
    m4v.clear();
    for (int k = 0; k < n; ++k) {
        const mhip_aln_result& a = res[k];
        if (!a.ok) continue;
        const mhip_candidate& c = cands[k];
        const mhip_aln_job j = job_of_candidate(c, q_local, T.ref_start_id);
        const int ssize = T.ref_offs[j.sid_local].size;
        M4Record m;     // fill_m4record, pw_impl.cpp:467-506
        m.qid = c.readno;
        m.sid = qid;
        m.ident = a.columns == 0 ? 0.0 : 100.0 * a.matches / a.columns;   // OutputStore::calc_ident / XdropAligner::calc_ident
        m.vscore = c.score;
        m.qdir = 0;
        m.qoff = a.target_start;
        m.qend = a.target_end;
        m.qsize = ssize;
        m.ssize = qsize;
        m.qext = j.sstart;
        if (c.chain == 0) { m.sdir = 0; m.soff = a.query_start; m.send = a.query_end; m.sext = j.qstart; }
        else { m.sdir = 1; m.soff = qsize - a.query_end; m.send = qsize - a.query_start; m.sext = qsize - 1 - j.qstart; }
        m4v.push_back(m);
    }
    // append_m4v, pw_impl.cpp:576-610
    std::sort(m4v.begin(), m4v.end(), CmpM4ByQidAndOvlpSize());
    const int nm = (int)m4v.size();
    S.valid.assign((size_t)nm, 1);
    for (int i = 0; i < nm;) {
        int e = i + 1;
        while (e < nm && m4v[(size_t)e].qid == m4v[(size_t)i].qid) ++e;
        if (e - i > 1) check_records_containment(m4v.data(), i, e, S.valid);
        i = e;
    }
    char line[320];
    for (int i = 0; i < nm; ++i) {
        if (!S.valid[(size_t)i]) continue;
        const M4Record& m = m4v[(size_t)i];
        int w = snprintf(line, 256, "%lld\t%lld\t%g\t%d\t%d\t%lld\t%lld\t%lld\t%d\t%lld\t%lld\t%lld", (long long)m.qid,
                         (long long)m.sid, m.ident, m.vscore, m.qdir, (long long)m.qoff, (long long)m.qend,
                         (long long)m.qsize, m.sdir, (long long)m.soff, (long long)m.send, (long long)m.ssize);
        if (gapped) w += snprintf(line + w, 64, "\t%lld\t%lld", (long long)m.qext, (long long)m.sext);
        line[w++] = '\n';
        o.append(line, (size_t)w);
        if (recs)
            recs->push_back(M4Rec{(int32_t)m.qid, (int32_t)m.sid, m.vscore, m.qdir, (int32_t)m.qoff, (int32_t)m.qend, (int32_t)m.qsize, m.sdir,
                                  (int32_t)m.soff, (int32_t)m.send, (int32_t)m.ssize, (int32_t)m.qext, (int32_t)m.sext});
    }
}
