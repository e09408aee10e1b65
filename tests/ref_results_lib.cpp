// mecat_amd/host/ref_results.{h,cpp} and ref_reads.{h,cpp} behind a C interface for the tests (compiled by tests/ref_ext_cases.py, linked
// with libmecat_hip.so).
#include <string.h>

#include <string>
#include <vector>

#include "../mecat_amd/host/ref_reads.cpp"
#include "../mecat_amd/host/ref_results.cpp"

extern "C" {

// text: the reads' letters one behind the other; -> num_bases, or -1
int64_t rr_pack(const char* text, const int* lens, int n, uint8_t* pac, uint8_t* nplane, int32_t* offs) {
    std::vector<const char*> seqs((size_t)n);
    const char* p = text;
    for (int i = 0; i < n; ++i) { seqs[(size_t)i] = p; p += lens[i]; }
    RefReads r;
    if (!ref_reads_pack(seqs.data(), lens, n, &r)) return -1;
    memcpy(pac, r.pac.data(), r.pac.size());
    memcpy(nplane, r.nplane.data(), r.nplane.size());
    memcpy(offs, r.reads.data(), r.reads.size() * sizeof(mhip_offset_t));
    return r.num_bases;
}

int rr_strings(const mhip_ref_result* r, const uint32_t* cols, const uint8_t* reads_pac, const uint8_t* reads_nplane, int64_t read_off, const uint8_t* ref_pac,
               char* qmap, char* smap) {
    std::string q, s;
    if (!ref_result_strings(*r, cols, reads_pac, reads_nplane, read_off, ref_pac, &q, &s)) return 0;
    memcpy(qmap, q.data(), q.size());
    memcpy(smap, s.data(), s.size());
    return 1;
}

int rr_record(int read_id, const mhip_ref_result* r, const char* qmap, const char* smap, char* out, int cap) {
    const std::string t = ref_result_record(read_id, *r, qmap, smap);
    if ((int)t.size() > cap) return -1;
    memcpy(out, t.data(), t.size());
    return (int)t.size();
}

void rr_align_info(const mhip_ref_result* r, int id, int64_t out[10]) {
    const RefAlignInfo a = ref_result_align_info(*r, id);
    out[0] = a.qoff; out[1] = a.qend; out[2] = a.parent_id; out[3] = a.id; out[4] = a.prev_id; out[5] = a.next_id; out[6] = a.valid; out[7] = a.qdir;
    out[8] = a.soff; out[9] = a.send;
}

}  // extern "C"
