// cns_groups.h — a partition file's records as the templates of one mhip_cns_correct_templates call: the order the reference's walks
// see, and its two gates in front of a template.  Plain host C++ (mecat2cns' driver; tests/cns_groups_lib.cpp reaches it for the tests).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mecat_hip.h"

struct CnsCmpBySid {      // CmpExtensionCandidateBySid, reads_correction_aux.cpp:81-87
    bool operator()(const mhip_ext_candidate& a, const mhip_ext_candidate& b) const { return a.sid < b.sid; }
};

// recs[0 .. n) as loaded from the file: sorted by sid with std::sort over the WHOLE array (unstable, :102 — the same call on the same
// bytes gives the reference's order, which for an m4 template of at most max_added records is the acceptance order), grouped by sid, the
// groups the reference skips dropped (fewer than min_cov records; ssize < min_size * 0.95 in double: reads_correction_can.cpp:32-33,
// reads_correction_m4.cpp:21-22) and the kept ones moved to the front.  -> tmpl_begin [templates + 1]; dropped[0 / 1] count the gates
inline std::vector<int64_t> cns_group_templates(mhip_ext_candidate* recs, size_t n, int min_cov, long long min_size, int64_t dropped[2]) {
    std::sort(recs, recs + n, CnsCmpBySid());
    std::vector<int64_t> tb(1, 0);
    size_t kept = 0;
    dropped[0] = dropped[1] = 0;
    for (size_t i = 0, j; i < n; i = j) {
        j = i + 1;
        while (j < n && recs[j].sid == recs[i].sid) ++j;
        if ((long long)(j - i) < (long long)min_cov) { ++dropped[0]; continue; }
        if ((double)recs[i].ssize < (double)min_size * 0.95) { ++dropped[1]; continue; }
        if (kept != i) std::copy(recs + i, recs + j, recs + kept);
        kept += j - i;
        tb.push_back((int64_t)kept);
    }
    return tb;
}
