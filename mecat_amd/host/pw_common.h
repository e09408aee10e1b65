// pw_common.h — what every part of the mecat2pw driver uses: the fatal-error macros (with the failure marker of a multi-process run), the
// reference's timers, the clock and the environment reader.
#pragma once

#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/time.h>
#include <unistd.h>

#include <string>
#include <thread>
#include <vector>

#include "mecat_hip.h"

// multi-process runs: a rank that dies leaves this marker so that the ranks waiting for its files stop too
inline char g_fail_marker[1024] = "";
inline void leave_fail_marker() {
    if (!g_fail_marker[0]) return;
    const int fd = open(g_fail_marker, O_CREAT | O_WRONLY, 0644);
    if (fd >= 0) close(fd);
}
#define DIE(...)                                                  \
    do {                                                          \
        fprintf(stderr, "[%s, %u] ", __func__, __LINE__);         \
        fprintf(stderr, __VA_ARGS__);                             \
        fprintf(stderr, "\n");                                    \
        leave_fail_marker();                                      \
        abort();                                                  \
    } while (0)
#define MCHK(call)                                                 \
    do {                                                           \
        if ((call) != 0) DIE("%s failed: %s", #call, mhip_last_error()); \
    } while (0)

inline double now_s() {
    struct timeval t;
    gettimeofday(&t, NULL);
    return t.tv_sec + 1e-6 * t.tv_usec;
}

inline int env_int(const char* a, const char* b, int dflt) {
    const char* e = getenv(a);
    if (!e && b) e = getenv(b);
    return e ? atoi(e) : dflt;
}

struct ScopedTimer {   // DynamicTimer, common/defs.h:175-191
    std::string name;
    double t0;
    explicit ScopedTimer(const std::string& n) : name(n) { fprintf(stderr, "[%s] begins.\n", name.c_str()); t0 = now_s(); }
    ~ScopedTimer() { fprintf(stderr, "[%s] takes %.2f secs.\n", name.c_str(), now_s() - t0); }
};

// extra phase timings on stderr, only with MECAT_TRACE set (the reference prints none of these)
struct TraceTimer {
    const char* name;
    double t0;
    bool on;
    explicit TraceTimer(const char* n) : name(n), t0(now_s()), on(getenv("MECAT_TRACE") != NULL) {}
    ~TraceTimer() { if (on) fprintf(stderr, "[trace] %-16s %.3f s\n", name, now_s() - t0); }
};

template <typename F>
static void run_threads(int nt, F f) {
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(f, t);
    f(0);
    for (auto& x : th) x.join();
}
