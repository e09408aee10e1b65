// mecat_amd/host/ref_genome.{h,cpp} behind a C interface for the tests (compiled by tests/ref_cand_cases.py, linked with libmecat_hip.so).
#include <string.h>

#include "../mecat_amd/host/ref_genome.cpp"

extern "C" {

// -> a handle, or NULL with the message in err (cap bytes)
void* rg_parse(const char* text, int64_t n, char* err, int cap) {
    RefGenome* g = new RefGenome();
    std::string e;
    if (!ref_genome_parse(text, (size_t)n, g, &e)) {
        snprintf(err, (size_t)cap, "%s", e.c_str());
        delete g;
        return nullptr;
    }
    return g;
}
void rg_free(void* h) { delete (RefGenome*)h; }
// sizes: num_bases, reads, chrindex bytes, chromosomes
void rg_sizes(void* h, int64_t out[4]) {
    const RefGenome* g = (const RefGenome*)h;
    out[0] = g->num_bases; out[1] = (int64_t)g->reads.size(); out[2] = (int64_t)g->chrindex.size(); out[3] = (int64_t)g->chroms.size();
}
void rg_copy(void* h, uint8_t* pac, uint8_t* nplane, int32_t* reads, char* chrindex) {
    const RefGenome* g = (const RefGenome*)h;
    memcpy(pac, g->pac.data(), g->pac.size());
    memcpy(nplane, g->nplane.data(), g->nplane.size());
    memcpy(reads, g->reads.data(), g->reads.size() * sizeof(mhip_offset_t));
    memcpy(chrindex, g->chrindex.data(), g->chrindex.size());
}
int rg_upload(void* ctx, void* h, void** vol, void** idx) {
    return ref_genome_upload((mhip_ctx*)ctx, *(const RefGenome*)h, (mhip_volume**)vol, (mhip_index**)idx);
}

}  // extern "C"
