// ref_reads.cpp — see ref_reads.h
#include "ref_reads.h"

namespace {

// get_dna_encode_table followed by `if (c > 3) c = 0`; plane: 3 unless the letter is an upper-case A, C, G or T
inline void read_code(unsigned char c, int* code, int* plane) {
    *plane = 3;
    switch (c) {
        case 'A': *code = 0; *plane = 0; break;
        case 'C': *code = 1; *plane = 0; break;
        case 'G': *code = 2; *plane = 0; break;
        case 'T': *code = 3; *plane = 0; break;
        case 'c': *code = 1; break;
        case 'g': *code = 2; break;
        case 't': *code = 3; break;
        default: *code = 0; break;
    }
}

}  // namespace

bool ref_reads_pack(const char* const* seqs, const int* lens, int n, RefReads* r) {
    *r = RefReads();
    int64_t tot = 0;
    for (int i = 0; i < n; ++i) tot += (int64_t)lens[i] + 1;
    if (tot > 0x7fffffff - 4096) return false;
    r->num_bases = tot;
    r->pac.assign((size_t)(tot + 3) / 4, 0);
    r->nplane.assign((size_t)(tot + 3) / 4, 0);
    int64_t p = 0;
    for (int i = 0; i < n; ++i) {
        r->reads.push_back(mhip_offset_t{(int32_t)p, (int32_t)lens[i]});
        for (int j = 0; j < lens[i]; ++j, ++p) {
            int c, pl;
            read_code((unsigned char)seqs[i][j], &c, &pl);
            const int sh = (int)((~p & 3) << 1);
            r->pac[(size_t)p >> 2] |= (uint8_t)(c << sh);
            r->nplane[(size_t)p >> 2] |= (uint8_t)(pl << sh);
        }
        ++p;      // the pad base
    }
    return true;
}

int ref_reads_upload(mhip_ctx* ctx, const RefReads& r, mhip_volume** vol) {
    *vol = nullptr;
    if (mhip_volume_upload(ctx, r.pac.data(), r.reads.data(), (int)r.reads.size(), (int)r.num_bases, 0, vol)) return -1;
    if (mhip_volume_set_nplane(ctx, *vol, r.nplane.data())) {
        mhip_volume_free(*vol);
        *vol = nullptr;
        return -1;
    }
    return 0;
}
