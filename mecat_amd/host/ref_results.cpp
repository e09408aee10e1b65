// ref_results.cpp — see ref_results.h
#include "ref_results.h"

#include <stdio.h>

bool ref_result_strings(const mhip_ref_result& r, const uint32_t* cols, const uint8_t* reads_pac, const uint8_t* reads_nplane, int64_t read_off,
                        const uint8_t* ref_pac, std::string* qmap, std::string* smap) {
    static const char dt[] = "ACGT-";
    qmap->assign((size_t)r.cols, '-');
    smap->assign((size_t)r.cols, '-');
    int qpos = r.qb;
    int64_t spos = r.sb;
    for (int c = 0; c < r.cols; ++c) {
        const int op = (int)((cols[c >> 4] >> ((c & 15) << 1)) & 3u);
        if (op == 3) return false;
        if (op != 1) {
            if (qpos >= r.qe) return false;
            // strand position p of the reverse strand is letter qs - 1 - p, complemented unless it is on the N plane (ref_reads.h)
            const int64_t at = read_off + (r.chain ? r.qs - 1 - qpos : qpos);
            int code = ref_packed_code(reads_pac, at);
            if (r.chain && !(reads_nplane && ref_packed_code(reads_nplane, at))) code = 3 - code;
            (*qmap)[(size_t)c] = dt[code];
            ++qpos;
        }
        if (op != 2) {
            if (spos >= r.se) return false;
            (*smap)[(size_t)c] = dt[ref_packed_code(ref_pac, spos)];
            ++spos;
        }
    }
    return qpos == r.qe && spos == r.se;
}

std::string ref_result_record(int read_id, const mhip_ref_result& r, const std::string& qmap, const std::string& smap) {
    char head[160];
    snprintf(head, sizeof(head), "%d\t%c\t%d\t%d\t%d\t%d\t%ld\t%ld\n", read_id, r.chain ? 'R' : 'F', r.vscore, r.qb, r.qe, r.qs, (long)r.sb, (long)r.se);
    return std::string(head) + qmap + "\n" + smap + "\n";
}

RefAlignInfo ref_result_align_info(const mhip_ref_result& r, int id) {
    RefAlignInfo a;
    a.qoff = r.qb;
    a.qend = r.qe;
    a.qdir = r.chain ? 'R' : 'F';
    a.soff = (long)r.sb;
    a.send = (long)r.se;
    a.valid = 1;
    a.id = id;
    a.prev_id = a.next_id = a.parent_id = -1;
    return a;
}

bool ref_read_records(int read_id, const int32_t* out_slots, int out_count, const RefResultSet& first, const RefResultSet& rescue,
                      const uint8_t* reads_pac, const uint8_t* reads_nplane, int64_t read_off, const uint8_t* ref_pac, std::string* out) {
    out->clear();
    std::string qmap, smap;
    for (int i = 0; i < out_count; ++i) {
        const int s = out_slots[i];
        const RefResultSet& set = s < first.count ? first : rescue;
        const int k = s < first.count ? s : s - first.count;
        if (k < 0 || k >= set.count || !set.res[k].ok) return false;
        if (!ref_result_strings(set.res[k], set.words + set.offs[k], reads_pac, reads_nplane, read_off, ref_pac, &qmap, &smap)) return false;
        *out += ref_result_record(read_id, set.res[k], qmap, smap);
    }
    return true;
}
