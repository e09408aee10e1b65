// mecat_amd/host/ref_results.{h,cpp}'s ref_read_records behind a C interface for the tests (compiled by tests/ref_rescue_cases.py).
#include <string.h>

#include <string>

#include "../mecat_amd/host/ref_results.cpp"

extern "C" {

// -> the bytes' length, -1 when the function refuses, -2 when they do not fit
int64_t rrr_read_records(int read_id, const int32_t* out_slots, int out_count, const mhip_ref_result* first, const uint64_t* first_offs, const uint32_t* first_words,
                         int maxc, const mhip_ref_result* rescue, const uint64_t* rescue_offs, const uint32_t* rescue_words, int tries, const uint8_t* reads_pac,
                         const uint8_t* reads_nplane, int64_t read_off, const uint8_t* ref_pac, char* out, int64_t cap) {
    RefResultSet a, b;
    a.res = first; a.offs = first_offs; a.words = first_words; a.count = maxc;
    b.res = rescue; b.offs = rescue_offs; b.words = rescue_words; b.count = tries;
    std::string t;
    if (!ref_read_records(read_id, out_slots, out_count, a, b, reads_pac, reads_nplane, read_off, ref_pac, &t)) return -1;
    if ((int64_t)t.size() > cap) return -2;
    memcpy(out, t.data(), t.size());
    return (int64_t)t.size();
}

}  // extern "C"
