// cns_slices_check.cpp — concat_slices and parallel_memcpy (mecat_amd/csrc/cns_slices.h) against a naive concatenation, on seeded random
// slice sets: a stand-alone program for the sanitizers (test_cns_slices_cpu.py builds it with -fsanitize=address,undefined).
// Exit 0 when every case agrees; the sanitizers abort on the first finding.
#define CNS_SLICES_STANDALONE
#include "cns_slices.h"

#include <stdio.h>

#include <random>

namespace {

std::mt19937_64 rng(20261);
int64_t pick(int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); }

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { fprintf(stderr, "case %d, line %d: %s\n", id, __LINE__, #cond); return false; } \
    } while (0)

bool one_case(int id) {
    const int kinds[] = {0, 1, 2, (int)pick(3, 12)};
    const int ns = kinds[pick(0, 3)];
    const size_t elems[] = {1, 16, 32};
    const size_t elem = elems[pick(0, 2)];
    const bool windows = pick(0, 3) != 0;          // slices own windows (pieces, consensus); else plain records (segments, windows)
    std::vector<SliceOut> store((size_t)ns);
    std::vector<SliceOut*> slices;
    std::vector<unsigned char> want_data;
    std::vector<int64_t> want_begin;
    std::vector<const void*> addr;
    for (SliceOut& s : store) {
        slices.push_back(&s);
        const bool with_begin = windows && pick(0, 3) != 0;
        s.n = windows ? (pick(0, 4) == 0 ? 0 : pick(1, 20)) : 0;
        int64_t count = windows ? 0 : pick(0, 30);
        std::vector<int64_t> local((size_t)s.n + 1, 0);
        if (with_begin) {
            for (int64_t i = 0; i < s.n; ++i) local[(size_t)i + 1] = local[(size_t)i] + (pick(0, 2) == 0 ? 0 : pick(1, 5));
            count = local[(size_t)s.n];
            s.begin.reset((int64_t*)malloc(sizeof(int64_t) * local.size()));
            memcpy(s.begin.get(), local.data(), sizeof(int64_t) * local.size());
        }
        for (int64_t i = 0; i < s.n; ++i) want_begin.push_back((int64_t)(want_data.size() / elem) + local[(size_t)i]);
        if (with_begin || !windows) {                // (a slice with windows and no begin[] produced nothing: no buffer either)
            s.cap = count + (pick(0, 1) ? pick(1, 10) : 0);
            s.count = windows ? -7 : count;          // (with begin[] the count is read from it)
            s.data.reset(malloc(std::max<size_t>(elem * (size_t)s.cap, 1)));
            unsigned char* d = (unsigned char*)s.data.get();
            for (size_t i = 0; i < elem * (size_t)s.cap; ++i) d[i] = (unsigned char)rng();
            want_data.insert(want_data.end(), d, d + elem * (size_t)count);
        }
        addr.push_back(s.data.get());
    }
    want_begin.push_back((int64_t)(want_data.size() / elem));
    // one refusal in some cases
    int expect = CONCAT_OK;
    if (ns > 0 && pick(0, 5) == 0) {
        SliceOut& s = store[(size_t)pick(0, ns - 1)];
        const int kind = (int)pick(0, 2);
        if (kind == 0) { s.bad = pick(1, 9); expect = CONCAT_BAD_FLAG; }
        else if (kind == 1 && s.begin) { s.begin.get()[0] = 1; expect = CONCAT_COUNTS; }
        else if (kind == 2 && s.begin && s.begin.get()[s.n] > 0) { s.cap = s.begin.get()[s.n] - 1; expect = CONCAT_COUNTS; }
    }
    CnsBuf<void> data;
    CnsBuf<int64_t> begin;
    int64_t total = -1, counts[2] = {-1, -1};
    const int rc = concat_slices(slices, elem, (int)pick(1, 4), &data, windows ? &begin : nullptr, &total, counts);
    CHECK(rc == expect);
    if (rc == CONCAT_COUNTS) CHECK(counts[1] >= 0 && counts[0] != -1);
    if (rc != CONCAT_OK) return true;
    CHECK(total == (int64_t)(want_data.size() / elem) && data);
    CHECK(want_data.empty() || memcmp(data.get(), want_data.data(), want_data.size()) == 0);
    if (windows) CHECK(begin && memcmp(begin.get(), want_begin.data(), sizeof(int64_t) * want_begin.size()) == 0);
    if (ns == 1 && addr[0]) CHECK(data.get() == addr[0] && !store[0].data);          // one slice: its buffer is the result, no copy
    else for (int k = 0; k < ns; ++k) CHECK(store[(size_t)k].data.get() == addr[(size_t)k] && data.get() != addr[(size_t)k]);
    return true;
}

bool big_copy() {          // more than two 64 MB pieces and an odd tail, on four threads
    const int id = -1;
    const size_t bytes = ((size_t)130 << 20) + 12345;
    std::vector<unsigned char> src(bytes), dst(bytes + 1, 0xee);
    for (size_t i = 0; i < bytes; ++i) src[i] = (unsigned char)(i * 2654435761u >> 13);
    parallel_memcpy(dst.data(), src.data(), bytes, 4);
    CHECK(memcmp(dst.data(), src.data(), bytes) == 0 && dst[bytes] == 0xee);
    parallel_memcpy(dst.data(), nullptr, 0, 4);
    return true;
}

}  // namespace

int main() {
    for (int id = 0; id < 4000; ++id)
        if (!one_case(id)) return 1;
    if (!big_copy()) return 1;
    printf("cns_slices_check: 4000 slice sets and the large copy agree\n");
    return 0;
}
