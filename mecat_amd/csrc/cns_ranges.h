// cns_ranges.h — mecat2cns' effective ranges of a template read: plain host C++ without any HIP, so that it can be built and run on
// its own (the accept replay of cns_accept.hip and the test hook of cns_plan.hip both call it).
//
// Reference: get_effective_ranges, mecat2cns/mecat_correction.cpp:118-153, called for PacBio at :445-447 with the (soff, send) of the
// accepted alignments in accept order (CnsAlns::get_mapping_ranges); nanopore takes the whole read instead (:508-509), as do the
// m4 variants (:357).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

// mranges: (start, end) of the accepted alignments (sorted in place, as the reference sorts its copy); read_size: bases of the
// template; the ranges are APPENDED to `out` as (start, end) pairs.  A template without bases (no candidates: the reference never
// looks at it) has no range.
inline void cns_effective_ranges(std::vector<std::pair<int32_t, int32_t>>& mranges, int read_size, int tech, int min_size, std::vector<int32_t>& out) {
    if (read_size <= 0) return;
    if (tech != 0) { out.push_back(0); out.push_back(read_size); return; }          // :509 (:357)
    if (mranges.empty()) return;                                                     // :122
    for (const auto& m : mranges)                                                    // :124-129: one alignment spans the read but <= 500 bases on either side
        if (m.first <= 500 && read_size - m.second <= 500) { out.push_back(0); out.push_back(read_size); return; }
    std::sort(mranges.begin(), mranges.end(), [](const std::pair<int32_t, int32_t>& a, const std::pair<int32_t, int32_t>& b) {
        return a.first == b.first ? a.second > b.second : a.first < b.first;          // CmpMappingRangeBySoff, :110-116
    });
    const int nr = (int)mranges.size();
    const double need = min_size * 0.95;                                             // `right - left >= min_size * 0.95`, :142 / :148, in double
    int i = 0, left = mranges[0].first;
    while (i < nr) {
        int j = i + 1;
        while (j < nr && mranges[(size_t)j].second <= mranges[(size_t)i].second) ++j;          // contained ranges, :138
        if (j == nr) {
            const int right = mranges[(size_t)i].second;
            if ((double)(right - left) >= need) { out.push_back(left); out.push_back(right); }
            break;
        }
        if (mranges[(size_t)i].second - mranges[(size_t)j].first < 1000) {                        // :145-150
            const int right = std::min(mranges[(size_t)i].second, mranges[(size_t)j].first);
            if ((double)(right - left) >= need) { out.push_back(left); out.push_back(right); }
            left = std::max(mranges[(size_t)i].second, mranges[(size_t)j].first);
        }
        i = j;
    }
}

// the smallest n with (double)n >= 0.95 * min_size: `end - beg >= 0.95 * min_size` (consensus_worker, :228) as an integer compare
inline int cns_plan_min_run(int min_size) {
    const double x = 0.95 * min_size;
    int n = (int)x;
    while ((double)n < x) ++n;
    while (n > 0 && (double)(n - 1) >= x) --n;
    return n;
}
