// cns_hostbuf.hip — the pool behind the accept stage's result buffers (cns_hostbuf.h, mhip_cns_free, mhip_cns_release_parked).
//
// The strings of a batch are gigabytes (24 GB at config 2), and pages that are touched for the first time cost more than the copy that
// fills them.  So the library keeps ONE released string buffer and hands it out again when the next batch fits it (mecat2cns works through
// its partitions batch after batch): pages that are mapped already.  mhip_cns_free parks a buffer it knows instead of freeing it; a larger
// request replaces the parked one.
#include <stdlib.h>
#include <sys/mman.h>

#include <algorithm>
#include <set>

#include "common.h"
#include "cns_hostbuf.h"
#include "cns_slices.h"

namespace {
std::mutex g_strbuf_mu;
char* g_strbuf_parked = nullptr;          // released, reusable
size_t g_strbuf_parked_cap = 0;
std::map<void*, size_t> g_strbuf_out;     // handed to a caller: address -> capacity
std::set<void*> g_strbuf_reg;             // page-locked (hipHostRegister): the copy engine fills them without a staging copy, asynchronously
void strbuf_free(void* p) {               // (g_strbuf_mu held or not: only the set is shared)
    if (!p) return;
    bool reg;
    { std::lock_guard<std::mutex> lk(g_strbuf_mu); reg = g_strbuf_reg.erase(p) != 0; }
    if (reg) (void)hipHostUnregister(p);
    free(p);
}
// cap bytes (a multiple of 2 MB), touched and page-locked; registered buffers are noted in g_strbuf_reg
void* locked_alloc(size_t cap, int num_threads) {
    void* p = nullptr;
    const size_t two_mb = (size_t)2 << 20;
    if (posix_memalign(&p, two_mb, cap) != 0) return nullptr;
    (void)madvise(p, cap, MADV_HUGEPAGE);
    // first touch on the host threads (huge pages: 8 GB in 30 ms on 32 threads), then page-locked — 70 ms for 8 GB of touched pages, against
    // 0.4 s untouched and 1.9 s for a hipHostMalloc of the size (tools/dev/probes/pin_probe.hip)
    parallel_for((int64_t)(cap / two_mb), num_threads, [&](int64_t pg) { ((volatile char*)p)[(size_t)pg * two_mb] = 0; });
    const bool reg = hipHostRegister(p, cap, hipHostRegisterDefault) == hipSuccess;
    if (!reg) (void)hipGetLastError();      // stays pageable: the copies still work, through the runtime's staging
    if (reg) { std::lock_guard<std::mutex> lk(g_strbuf_mu); g_strbuf_reg.insert(p); }
    return p;
}
}  // namespace

char* strbuf_get(size_t bytes, int num_threads) {
    {
        std::lock_guard<std::mutex> lk(g_strbuf_mu);
        if (g_strbuf_parked && g_strbuf_parked_cap >= bytes) {
            char* p = g_strbuf_parked;
            g_strbuf_out[p] = g_strbuf_parked_cap;
            g_strbuf_parked = nullptr;
            g_strbuf_parked_cap = 0;
            return p;
        }
    }
    const size_t two_mb = (size_t)2 << 20, cap = (bytes + bytes / 16 + two_mb - 1) & ~(two_mb - 1);
    void* p = locked_alloc(cap, num_threads);
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(g_strbuf_mu);
    g_strbuf_out[p] = cap;
    return (char*)p;
}

void* result_alloc(size_t bytes, int num_threads) {
    if (bytes < ((size_t)64 << 20)) return malloc(std::max<size_t>(bytes, 1));
    const size_t two_mb = (size_t)2 << 20;
    return locked_alloc((bytes + two_mb - 1) & ~(two_mb - 1), num_threads);
}

extern "C" {

void mhip_cns_free(void* p) {
    if (!p) return;
    void* to_free = p;
    {
        std::lock_guard<std::mutex> lk(g_strbuf_mu);
        auto it = g_strbuf_out.find(p);
        if (it != g_strbuf_out.end()) {
            const size_t cap = it->second;
            g_strbuf_out.erase(it);
            if (cap > g_strbuf_parked_cap) {      // park this one, free what was parked (the smaller of the two)
                to_free = g_strbuf_parked;
                g_strbuf_parked = (char*)p;
                g_strbuf_parked_cap = cap;
            }
        }
    }
    strbuf_free(to_free);      // (a plain malloc'ed buffer — the accepted records, small string buffers — is just freed)
}

// gives the parked string buffer (see above) back to the system; buffers still in a caller's hands are not touched
void mhip_cns_release_parked(void) {
    void* p;
    {
        std::lock_guard<std::mutex> lk(g_strbuf_mu);
        p = g_strbuf_parked;
        g_strbuf_parked = nullptr;
        g_strbuf_parked_cap = 0;
    }
    strbuf_free(p);
}

}  // extern "C"
