// cns_replay.h — the accept decisions of one template read, replayed over the device's alignment results: plain host C++ without any
// HIP (cns_accept.hip runs it per template on host threads).
//
// Reference: the candidate loop of consensus_one_read_can_pacbio / _nanopore, mecat2cns/mecat_correction.cpp:419-443 (:482-506), and
// as a second rule set the overlap loop of consensus_one_read_m4_pacbio / _nanopore, :261-293 (:322-354).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <set>
#include <vector>

#include "mecat_hip.h"

struct CnsReplayRules {
    int max_ext;          // candidates looked at per template, :412
    int max_added;        // alignments accepted per template, :407 ; MAX_CNS_OVLPS, reads_correction_aux.h:32
    double ratio;         // min_mapping_ratio - 0.02, :406
};

// Template t's candidates are cands[tmpl_begin[t] .. tmpl_begin[t + 1]) in the order of the reference's walk; candidate i (< max_ext) was
// aligned as job jfirst[t] + i, with its result at that index of res[].  -> the accepted job indices, in acceptance order
inline std::vector<int32_t> cns_replay_template(const mhip_ext_candidate* cands, const int64_t* tmpl_begin, const mhip_cns_result* res, const int64_t* jfirst, int64_t t,
                                                const CnsReplayRules& rules) {
    std::vector<int32_t> acc;
    const int64_t b = tmpl_begin[t], n = tmpl_begin[t + 1] - b;
    if (n == 0) return acc;
    std::vector<uint8_t> cov((size_t)(cands[b].ssize > 1 ? cands[b].ssize : 1), 0);      // (every candidate's ssize is the template's length)
    std::set<int> used;
    int num_added = 0, num_ext = 0;
    for (int64_t i = 0; i < n && num_added < rules.max_added && num_ext < rules.max_ext; ++i) {
        ++num_ext;
        const mhip_ext_candidate& ec = cands[b + i];
        if (used.find(ec.qid) != used.end()) continue;                   // :424
        const int64_t ji = jfirst[t] + i;                                // i < max_ext here: the job exists
        const mhip_cns_result& r = res[ji];
        if (!r.ok) continue;
        const int oq = r.qend - r.qoff, qqs = (int)(ec.qsize * rules.ratio), os = r.send - r.soff, qss = (int)(ec.ssize * rules.ratio);      // :191-200
        if (!(oq >= qqs || os >= qss)) continue;
        int full = 0;                                                    // check_cov_stats, :372-386
        for (int p = r.soff; p < r.send; ++p) full += cov[(size_t)p] >= 20;
        if (!(r.send - r.soff >= full + 200)) continue;
        for (int p = r.soff; p < r.send; ++p) ++cov[(size_t)p];
        ++num_added;
        used.insert(ec.qid);
        acc.push_back((int32_t)ji);
    }
    return acc;
}

// ---- the m4 walk: a template's records are overlaps, not candidates

struct CnsReplayM4Rules {
    int max_added;        // overlaps aligned per template: 60, :259 ; MAX_CNS_OVLPS, :323
    bool check_ratio;     // nanopore: check_ovlp_mapping_range, :348 ; PacBio makes no such check, :286-287
    double ratio;         // min_mapping_ratio - 0.02, :320
};

struct CnsCmpOverlapSize {      // CompareOverlapByOverlapSize, :26-34: no tie-break
    bool operator()(const mhip_ext_candidate& a, const mhip_ext_candidate& b) const {
        return std::max(a.qend - a.qoff, a.send - a.soff) > std::max(b.qend - b.qoff, b.send - b.soff);
    }
};

// The order of the reference's walk over cands[0 .. n): as given with at most max_added records; with more, the WHOLE range sorted by
// overlap size (:271 / :332).  std::sort, not stable_sort: the reference sorts the same array with the same comparator and the same
// libstdc++ introsort, so records that tie come out in the reference's order exactly when the input order is the reference's.
// -> the records that become jobs: the first min(n, max_added)
inline int64_t cns_replay_m4_order(mhip_ext_candidate* cands, int64_t n, const CnsReplayM4Rules& rules) {
    if (n <= rules.max_added) return n;
    std::sort(cands, cands + n, CnsCmpOverlapSize());
    return rules.max_added;
}

// Template t's overlaps in walk order; overlap i (< min(n, max_added)) was aligned as job jfirst[t] + i.  Every one of them is accepted
// when its alignment succeeded and (check_ratio) covers enough of either read.  -> the accepted job indices, in acceptance order
inline std::vector<int32_t> cns_replay_template_m4(const mhip_ext_candidate* cands, const int64_t* tmpl_begin, const mhip_cns_result* res, const int64_t* jfirst, int64_t t,
                                                   const CnsReplayM4Rules& rules) {
    std::vector<int32_t> acc;
    const int64_t b = tmpl_begin[t], n = std::min<int64_t>(tmpl_begin[t + 1] - b, rules.max_added);
    for (int64_t i = 0; i < n; ++i) {
        const mhip_ext_candidate& ec = cands[b + i];
        const int64_t ji = jfirst[t] + i;
        const mhip_cns_result& r = res[ji];
        if (!r.ok) continue;
        if (rules.check_ratio) {                                         // :191-200
            const int oq = r.qend - r.qoff, qqs = (int)(ec.qsize * rules.ratio), os = r.send - r.soff, qss = (int)(ec.ssize * rules.ratio);
            if (!(oq >= qqs || os >= qss)) continue;
        }
        acc.push_back((int32_t)ji);
    }
    return acc;
}
