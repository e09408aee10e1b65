// pw_slabs_check.cpp — SlabQueue and the stage clocks of mecat_amd/host/pw_slabs.h (the mecat2pw driver's hand-over of slab buffers from
// the thread that drives the GPU to the thread that writes) with stub buffers and no library: a stand-alone program for
// ThreadSanitizer (test_pw_slabs_cpu.py builds it with -fsanitize=thread).  Exit 0 when every row behaved; ThreadSanitizer reports races.
#include "pw_slabs.h"

#include <stdio.h>

#include <atomic>
#include <random>

struct StubBuf {
    int filled = 0, written = 0;      // generation counters: the number (from 1) of the slab last put into / last written out of the buffer
};

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "row %d, line %d: %s\n", row, __LINE__, #cond); exit(1); } \
    } while (0)

static int g_snapshots_while_writing = 0;

static void one_row(int row, const std::vector<int>& slabs_per_cell, bool drain_after_cell) {
    std::mt19937 rng(1000u + (unsigned)row);
    int next_to_write = 1;              // writer thread only
    double format_sum = 0, write_sum = 0;
    std::atomic<int> written{0};
    SlabQueue<StubBuf> q([&](StubBuf& B, double* clk) {
        CHECK(B.filled == next_to_write);          // production order
        const double t0 = now_s();
        usleep(100 + rng() % 300);
        const double t1 = now_s();
        clk[ST_FORMAT] += t1 - t0;
        format_sum += t1 - t0;
        { StageClock sc(&clk[ST_WRITE]); B.written = B.filled; }
        write_sum += clk[ST_WRITE];
        ++next_to_write;
        written.store(B.written);
    });
    double last[ST_N] = {0, 0, 0, 0, 0, 0, 0, 0};
    int produced = 0;
    for (int n : slabs_per_cell) {
        for (int s = 0; s < n; ++s) {
            StubBuf& B = q.acquire();
            CHECK(&B == &q.slabs[produced & 1] && q.filled_so_far() == produced);
            CHECK(B.written == B.filled);          // never handed out while its previous slab is unwritten
            CHECK(B.filled == (produced >= 2 ? produced - 1 : 0));
            { StageClock sc(&q.gpu[ST_SEED]); B.filled = produced + 1; }
            ++produced;
            q.filled();
        }
        if (drain_after_cell) {
            q.drain();
            CHECK(written.load() == produced);
        }
        const bool busy_before = written.load() < produced;
        double st[ST_N];
        q.snapshot(st);
        if (busy_before && written.load() < produced) ++g_snapshots_while_writing;      // the writer was at work all through the snapshot
        for (int k = 0; k < ST_N; ++k) { CHECK(st[k] >= last[k]); last[k] = st[k]; }
    }
    q.close();
    q.close();          // (a second close is nothing)
    CHECK(written.load() == produced && next_to_write == produced + 1);
    double st[ST_N];
    q.snapshot(st);
    CHECK(st[ST_FORMAT] == format_sum && st[ST_WRITE] == write_sum);          // every slab's clocks arrived, once
    CHECK(st[ST_SEED] == q.gpu[ST_SEED] && st[ST_JOBS] == 0);
}

int main() {
    const std::vector<std::vector<int>> rows = {{1}, {2}, {1, 1, 5}, {3, 0, 2}};      // slabs per cell; the last has a cell with no reads
    int row = 0;
    for (int drain = 0; drain < 2; ++drain)
        for (const std::vector<int>& r : rows) one_row(row++, r, drain != 0);
    CHECK(g_snapshots_while_writing > 0);
    printf("%d rows, %d clock snapshots taken while the writer ran\n", row, g_snapshots_while_writing);
    return 0;
}
