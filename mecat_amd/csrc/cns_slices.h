// cns_slices.h — outputs of the accept stage whose length is known slice by slice only (segments, windows, pieces, consensus bytes),
// and the routine that puts the slices' parts behind one another.  Plain host C++ without any HIP; with CNS_SLICES_STANDALONE defined
// the buffers are plain malloc's, so that tests/cns_slices_check.cpp can run it under the sanitizers without the library.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <thread>
#include <vector>

#ifdef CNS_SLICES_STANDALONE
inline void* result_alloc(size_t bytes, int) { return malloc(std::max<size_t>(bytes, 1)); }
struct CnsFree { void operator()(void* p) const { free(p); } };
template <typename T> using CnsBuf = std::unique_ptr<T, CnsFree>;
#else
#include "cns_hostbuf.h"
#endif

template <typename F>
void parallel_for(int64_t n, int nthreads, F f) {
    nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(nthreads, n));
    std::atomic<int64_t> next{0};
    auto body = [&]() {
        for (;;) {
            const int64_t i = next.fetch_add(1);
            if (i >= n) return;
            f(i);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; ++t) th.emplace_back(body);
    body();
    for (auto& x : th) x.join();
}

// memcpy in pieces of 64 MB on up to `threads` threads (gigabytes at config 2)
inline void parallel_memcpy(void* dst, const void* src, size_t bytes, int threads) {
    const size_t part = (size_t)64 << 20;
    parallel_for((int64_t)((bytes + part - 1) / part), threads, [&](int64_t k) {
        const size_t o = (size_t)k * part;
        memcpy((char*)dst + o, (const char*)src + o, std::min(part, bytes - o));
    });
}

// One slice's part of such an output: `cap` elements of which the first `count` hold records.  With begin[] — [n + 1], the first element
// of each of the slice's n windows counted from the slice's first — count is begin[n], read at the hand-over (the copy lands late); a
// slice without begin[] has n windows that own nothing, or (n == 0) a count the host knows.
struct SliceOut {
    CnsBuf<void> data; CnsBuf<int64_t> begin;
    int64_t n = 0, count = 0, cap = 0;
    long long bad = 0;          // the kernels' flag, copied with the data: refused at the hand-over
};

enum { CONCAT_OK = 0, CONCAT_BAD_FLAG, CONCAT_COUNTS, CONCAT_NO_MEMORY };

// Every slice's records behind one another in *data (`elem` bytes each, *total of them) and, with `begin`, the windows' first elements
// moved from slice-local to batch-wide numbers: [sum of n + 1].  One slice with a buffer: the buffer is the result (cap-sized), no copy.
// CONCAT_COUNTS leaves the offending slice's count and cap in counts[2].
inline int concat_slices(const std::vector<SliceOut*>& slices, size_t elem, int threads, CnsBuf<void>* data, CnsBuf<int64_t>* begin, int64_t* total, int64_t counts[2]) {
    int64_t owners = *total = 0;
    for (SliceOut* s : slices) {
        if (s->bad) return CONCAT_BAD_FLAG;
        if (s->begin) {
            s->count = s->begin.get()[s->n];
            if (s->begin.get()[0] != 0 || s->count < 0 || s->count > s->cap) { counts[0] = s->count; counts[1] = s->cap; return CONCAT_COUNTS; }
        }
        *total += s->count;
        owners += s->n;
    }
    if (begin) begin->reset((int64_t*)malloc(sizeof(int64_t) * ((size_t)owners + 1)));
    if (slices.size() == 1 && slices[0]->data) *data = std::move(slices[0]->data);
    else {
        data->reset(result_alloc(elem * (size_t)*total, threads));
        size_t o = 0;
        if (*data) for (const SliceOut* s : slices) {
            parallel_memcpy((char*)data->get() + o, s->data.get(), elem * (size_t)s->count, threads);
            o += elem * (size_t)s->count;
        }
    }
    if (!*data || (begin && !*begin)) return CONCAT_NO_MEMORY;
    if (!begin) return CONCAT_OK;
    int64_t wo = 0, base = 0;
    for (const SliceOut* s : slices) {
        for (int64_t i = 0; i < s->n; ++i) begin->get()[wo + i] = base + (s->begin ? s->begin.get()[i] : 0);
        wo += s->n;
        base += s->count;
    }
    begin->get()[wo] = base;
    return CONCAT_OK;
}
