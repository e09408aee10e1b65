// scan.h — the single-workgroup array scan behind every stage that turns per-item counts into positions.
#pragma once

#include "common.h"

// One workgroup of 1024 threads.  store(i, base + load(0) + .. + load(i - 1)) for every i < n, tiles of 1024 with a running sum;
// returns base + the sum of all n values, to every thread.  n and base are uniform across the workgroup.  Each thread calls load(i) before
// store(i) for the same i and no thread touches another thread's i, so the scan may run in place.  Ends with a barrier (n <= 0: nothing is read, written or waited for).
// A tile: inclusive scan inside each wave, the sixteen wave totals to LDS, every thread adds the totals in front of its wave and all
// sixteen to its own copy of the running sum — two barriers per tile, none for the carry.
template <typename Acc, typename Load, typename Store>
__device__ __forceinline__ Acc scan_array_1024(long long n, Acc base, Load load, Store store) {
    __shared__ Acc wsum[16];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    Acc run = base;
    for (long long i0 = 0; i0 < n; i0 += 1024) {
        const long long i = i0 + threadIdx.x;
        const Acc v = i < n ? (Acc)load(i) : (Acc)0;
        Acc x = v;
        for (int o = 1; o < 64; o <<= 1) {
            const Acc y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        Acc off = run, tot = 0;
        for (int k = 0; k < 16; ++k) {
            if (k < w) off += wsum[k];
            tot += wsum[k];
        }
        if (i < n) store(i, off + x - v);
        run += tot;
        __syncthreads();
    }
    return run;
}
