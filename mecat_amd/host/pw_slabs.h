// pw_slabs.h — the two slab buffers of a grid row and their hand-over from the thread that drives the GPU to the thread that formats
// and writes, with the stage clocks both threads keep.  Nothing here calls the library: the page-locking of PinnedBuf goes through
// its `Pin` parameter.
#pragma once

#include <stdint.h>
#include <stdlib.h>
#include <sys/mman.h>

#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "pw_common.h"

struct HostVolume;      // volume.h

// growable array in page-locked host memory (contents are not preserved across a grow: every user refills it).  Pin::lock(p, bytes) /
// Pin::unlock(p) page-lock and release (the driver: mhip_host_register / mhip_host_unregister)
template <typename T, typename Pin>
struct PinnedBuf {
    // buffers that cross the PCIe link: 2 MB-aligned huge pages, touched here and then page-locked (mhip_host_register) — 100 MB in a few
    // milliseconds, where a hipHostMalloc of the size takes 25 - 60 ms (tools/dev/probes/pin_probe.hip)
    T* p = nullptr;
    size_t cap = 0, n = 0;
    bool locked = false;
    void release() {
        if (!p) return;
        if (locked) Pin::unlock(p);
        free(p);
        p = nullptr;
        locked = false;
    }
    ~PinnedBuf() { release(); }
    void resize(size_t want) {
        if (want > cap) {
            release();
            cap = want + want / 8 + 1024;
            const size_t huge = (size_t)2 << 20, bytes = (cap * sizeof(T) + huge - 1) & ~(huge - 1);
            void* q = nullptr;
            if (posix_memalign(&q, huge, bytes) != 0) DIE("out of memory (%zu bytes of transfer buffer)", bytes);
            (void)madvise(q, bytes, MADV_HUGEPAGE);
            for (size_t o = 0; o < bytes; o += huge) ((volatile char*)q)[o] = 0;
            locked = Pin::lock(q, bytes) == 0;      // (not locked: the copies still work, slower)
            p = (T*)q;
        }
        n = want;
    }
    T* data() { return p; }
    size_t size() const { return n; }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
};

template <typename Pin>
struct SlabBuf {
    PinnedBuf<mhip_candidate, Pin> cands;      // buffers that cross the PCIe link: page-locked
    PinnedBuf<int32_t, Pin> counts;
    PinnedBuf<mhip_aln_job, Pin> jobs;
    PinnedBuf<mhip_aln_result, Pin> res;
    std::vector<size_t> jfirst;       // first entry of read r's list in res[] (and in cands[] when packed)
    int rb = 0, nr = 0;
    const HostVolume* rd = NULL;      // the query volume the slab belongs to, and its number (the writer thread works across cells)
    int vid = 0;
    bool packed = false;              // cands[] holds only the occupied entries, read-major (one process); else [nr][maxc]
};

// MECAT_TRACE: seconds in seeding, job assembly, extension, formatting, writing (+ copies), page-locked buffers, waits for a slab
// buffer, device memory query
enum Stage { ST_SEED, ST_JOBS, ST_EXTEND, ST_FORMAT, ST_WRITE, ST_PIN, ST_WAIT, ST_MEMQ, ST_N };
struct StageClock {      // adds the life time of the object to *acc
    double* acc;
    double t0;
    explicit StageClock(double* a) : acc(a), t0(now_s()) {}
    ~StageClock() { *acc += now_s() - t0; }
    StageClock(const StageClock&) = delete;
};

// Two-stage pipeline over the slabs of a grid row: the owner's thread drives the GPU (seeding, job assembly, extension) for slab s + 1
// while the queue's thread formats and writes slab s (text assembly is per read and order preserving; one writer keeps the order).
// One writer for the whole row: the text of cell n's last slabs is assembled while cell n + 1 is being seeded (a slab carries the query
// volume it belongs to) — at `-j 0` a cell is one seeding call and then nothing but copies and formatting, which used to run with the GPU
// idle: 3 of the 29 s of config 5's 190 cells.  Slab s lives in buffer s & 1 (the two alternate across cells as well), is written
// before that buffer is handed out again, and slabs are written in the order they were filled.
// Clocks: `gpu` belongs to the owner's thread; the writer fills clocks of its own per slab (the array `write` is called with) and adds them
// to its totals under the mutex when the slab is done; snapshot() reads both under the mutex.
template <typename B>
class SlabQueue {
public:
    B slabs[2];
    double gpu[ST_N] = {0, 0, 0, 0, 0, 0, 0, 0};
    explicit SlabQueue(std::function<void(B&, double*)> write) : write_(std::move(write)), writer_([this]() { writer_loop(); }) {}
    ~SlabQueue() { close(); }
    int filled_so_far() const { return produced_; }      // slabs of the row so far (owner's thread)
    B& acquire() {      // the buffer of the next slab, once the slab that was in it has been written out
        StageClock sc(&gpu[ST_WAIT]);
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&]() { return consumed_ >= produced_ - 1; });
        return slabs[produced_ & 1];
    }
    void filled() {      // the buffer acquire() returned holds a whole slab: over to the writer
        { std::lock_guard<std::mutex> lk(m_); ++produced_; }
        cv_.notify_all();
    }
    void drain() {      // returns when every slab handed over has been written (what the slabs point to may go away then)
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&]() { return consumed_ >= produced_; });
    }
    void close() {      // lets the writer finish what is queued and joins it
        if (!writer_.joinable()) return;
        { std::lock_guard<std::mutex> lk(m_); closing_ = true; }
        cv_.notify_all();
        writer_.join();
    }
    void snapshot(double out[ST_N]) {      // both threads' clocks, summed
        std::lock_guard<std::mutex> lk(m_);
        for (int k = 0; k < ST_N; ++k) out[k] = gpu[k] + written_[k];
    }

private:
    void writer_loop() {
        for (;;) {
            int s;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&]() { return consumed_ < produced_ || closing_; });
                if (consumed_ >= produced_) return;
                s = consumed_;
            }
            double mine[ST_N] = {0, 0, 0, 0, 0, 0, 0, 0};
            write_(slabs[s & 1], mine);
            {
                std::lock_guard<std::mutex> lk(m_);
                for (int k = 0; k < ST_N; ++k) written_[k] += mine[k];
                ++consumed_;
            }
            cv_.notify_all();
        }
    }
    std::function<void(B&, double*)> write_;
    std::mutex m_;
    std::condition_variable cv_;
    int produced_ = 0, consumed_ = 0;
    bool closing_ = false;
    double written_[ST_N] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::thread writer_;      // (last member: it starts in the constructor and uses the others)
};
