// cns_groups_lib.cpp — TEST INFRASTRUCTURE: mecat2cns' grouping of a partition file's records (mecat_amd/cns/cns_groups.h: the whole-array
// std::sort by sid, the two gates) behind a C entry point, built by the tests into a temporary directory so that they hand
// mhip_cns_correct_templates the templates in the order the driver does.
#include "cns_groups.h"

extern "C" {
// recs: n x 13 int32, reordered in place -> the number of templates; tmpl_begin[templates + 1] (room for n + 1), dropped[2]
int64_t cns_groups_make(int32_t* recs, int64_t n, int min_cov, int64_t min_size, int64_t* tmpl_begin, int64_t* dropped) {
    const std::vector<int64_t> tb = cns_group_templates((mhip_ext_candidate*)recs, (size_t)n, min_cov, min_size, dropped);
    std::copy(tb.begin(), tb.end(), tmpl_begin);
    return (int64_t)tb.size() - 1;
}
}
