// pw_run.cpp — the multi-process protocol of mecat2pw (pw_run.h)
#include "pw_run.h"

#include <ctype.h>
#include <signal.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>

#include "pw_common.h"

static std::string run_token() {
    if (const char* e = getenv("MECAT_HIP_RUN_ID")) return std::string("x") + e;
    std::string t = "p" + std::to_string((long)getppid());
    if (const char* e = getenv("TORCHELASTIC_RUN_ID")) t += std::string("_") + e;
    if (const char* e = getenv("MASTER_PORT")) t += std::string("_") + e;
    // an elastic restart by the same launcher keeps all of the above: the restart count tells the attempts apart, so that a rank of
    // attempt k + 1 never accepts the split marker (communicator id, rows to do) attempt k left behind
    if (const char* e = getenv("TORCHELASTIC_RESTART_COUNT")) t += std::string("_r") + e;
    for (char& ch : t)
        if (!isalnum((unsigned char)ch) && ch != '_' && ch != '-') ch = '_';
    return t;
}

Run run_from_env(const char* wrk_dir) {
    Run run;
    run.world = std::max(1, env_int("MECAT_HIP_WORLD", "WORLD_SIZE", 1));
    run.rank = std::min(run.world - 1, std::max(0, env_int("MECAT_HIP_RANK", "RANK", 0)));
    run.t_start = now_s();
    run.rf.dir = wrk_dir;
    if (run.rf.dir.empty() || run.rf.dir[run.rf.dir.size() - 1] != '/') run.rf.dir += '/';
    run.rf.token = run_token();
    run.explicit_token = getenv("MECAT_HIP_RUN_ID") != NULL;
    run.wait_limit = env_int("MECAT_HIP_WAIT_S", NULL, 6 * 3600);
    return run;
}

static std::string to_hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}
static bool from_hex(const std::string& s, uint8_t* p, size_t n) {
    if (s.size() != 2 * n) return false;
    auto v = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; };
    for (size_t i = 0; i < n; ++i) {
        const int a = v(s[2 * i]), b = v(s[2 * i + 1]);
        if (a < 0 || b < 0) return false;
        p[i] = (uint8_t)(a * 16 + b);
    }
    return true;
}

void publish_split(const Run& run, const Split& s) {
    const std::string marker = run.rf.marker();
    FILE* m = fopen((marker + ".tmp").c_str(), "w");
    if (!m) DIE("cannot write '%s'", marker.c_str());
    fprintf(m, "%s %.3f %d %d %s\n", run.rf.token.c_str(), run.t_start, s.num_vols, s.cells ? 1 : 0, to_hex(s.comm_id, sizeof(s.comm_id)).c_str());
    for (int i : s.todo) fprintf(m, "%d ", i);
    fprintf(m, "\n");
    fclose(m);
    if (rename((marker + ".tmp").c_str(), marker.c_str()) != 0) DIE("cannot rename %s", marker.c_str());
}

// wait for THIS run's split: the marker carries the run token (and, for a token that was not given explicitly, must be
// younger than this process: a restart by the same parent would reuse the token)
void await_split(const Run& run, const char* wrk_dir, Split* s) {
    const std::string marker = run.rf.marker();
    for (;;) {
        FILE* m = fopen(marker.c_str(), "r");
        char tok[256] = "", hex[2 * MHIP_COMM_ID_BYTES + 8] = "";      // 264 bytes: %263s below
        double t0 = 0;
        int nv = 0, cl = 0;
        const bool ok = m && fscanf(m, "%255s %lf %d %d %263s", tok, &t0, &nv, &cl, hex) == 5;
        if (ok && run.rf.token == tok && (run.explicit_token || t0 > run.t_start - 120.0) && from_hex(hex, s->comm_id, sizeof(s->comm_id))) {
            int v;
            while (fscanf(m, "%d", &v) == 1) s->todo.push_back(v);
            fclose(m);
            s->num_vols = nv;
            s->cells = cl != 0;
            return;
        }
        if (m) fclose(m);
        if (now_s() - run.t_start > run.wait_limit)
            DIE("rank %d: no split marker of run '%s' in %s after %.0f s", run.rank, run.rf.token.c_str(), wrk_dir, run.wait_limit);
        usleep(20 * 1000);
    }
}

static double mtime_of(const struct stat& sb) { return (double)sb.st_mtim.tv_sec + 1e-9 * (double)sb.st_mtim.tv_nsec; }

// The stale-marker rule.  A token can be reused (a fixed MECAT_HIP_RUN_ID, ranks started by hand from one shell), and a failed attempt
// leaves every rank's failure marker and possibly a stale heartbeat behind.  Every rank removes its OWN failure marker when it
// starts, so a peer's marker says "the peer failed in the last attempt it started": younger than this process — this attempt, believed
// at once; older — either the attempt before (and the peer of this one has not started yet: it will remove it), or this attempt
// with the peer started, and dead, more than a launcher's skew before this rank (that peer also removed its heartbeat,
// so nothing else would ever notice).  The two are told apart by waiting: an older marker that is still there `grace` seconds
// after this rank started (MECAT_HIP_PEER_GRACE_S, default 120: the time after which a peer without a heartbeat counts as "not
// running" anyway, so a peer that is merely late — slow launcher, GPU lease wait, ranks started by hand — is not declared dead any
// earlier on account of a stale marker) is believed.  ("Younger" allows a second: st_mtime has one-second granularity on
// some file systems.)
static bool failure_marker_believed(const std::string& marker, double t_start) {
    struct stat sb;
    if (stat(marker.c_str(), &sb) != 0) return false;
    return mtime_of(sb) >= t_start - 1.0 || now_s() - t_start > env_int("MECAT_HIP_PEER_GRACE_S", NULL, 120);
}
bool peer_failed(const Run& run, int peer) { return failure_marker_believed(run.rf.failed(peer), run.t_start); }

// the thread's body.  The 60 s silence rule applies to a peer only once a heartbeat of THIS attempt has been seen from it.
static void beat_loop(std::atomic<bool>& stop, const std::string alive, const std::vector<std::string> peer_failed, const std::vector<std::string> peer_alive,
                      int rank, double t_start) {
    const bool watch = !getenv("MECAT_HIP_NO_WATCHDOG");
    std::vector<char> seen(peer_alive.size(), 0);
    while (!stop.load()) {
        const int fd = open(alive.c_str(), O_CREAT | O_WRONLY | O_TRUNC, 0644);
        if (fd >= 0) { (void)!write(fd, "1\n", 2); close(fd); }
        for (int i = 0; i < 20 && !stop.load(); ++i) {
            usleep(100 * 1000);
            if (!watch || i % 5) continue;
            for (size_t k = 0; k < peer_failed.size(); ++k) {
                struct stat sb;
                bool dead = failure_marker_believed(peer_failed[k], t_start);
                const char* why = "left a failure marker";
                if (!dead && stat(peer_alive[k].c_str(), &sb) == 0) {
                    if (mtime_of(sb) >= t_start - 1.0) seen[k] = 1;
                    if (seen[k] && now_s() - mtime_of(sb) > 60.0) { dead = true; why = "stopped responding"; }
                }
                if (dead && !stop.load()) {
                    fprintf(stderr, "[mecat2pw rank %d] a peer %s (%s): stopping\n", rank, why, peer_failed[k].c_str());
                    leave_fail_marker();
                    unlink(alive.c_str());
                    _exit(1);
                }
            }
        }
    }
    unlink(alive.c_str());
}

void Heartbeat::start(const Run& run) {
    if (run.world <= 1) return;
    snprintf(g_fail_marker, sizeof(g_fail_marker), "%s", run.rf.failed(run.rank).c_str());
    unlink(g_fail_marker);
    signal(SIGSEGV, [](int) { leave_fail_marker(); _exit(139); });
    signal(SIGTERM, [](int) { leave_fail_marker(); _exit(143); });
    signal(SIGABRT, [](int) { leave_fail_marker(); _exit(134); });      // the reader's and the splitter's ERROR() abort, like the reference's
    signal(SIGBUS, [](int) { leave_fail_marker(); _exit(135); });       // (an mmap'd input that shrank under the reader)
    std::vector<std::string> peer_failed, peer_alive;
    for (int r = 0; r < run.world; ++r)
        if (r != run.rank) { peer_failed.push_back(run.rf.failed(r)); peer_alive.push_back(run.rf.alive(r)); }
    t_ = std::thread(beat_loop, std::ref(stop_), run.rf.alive(run.rank), peer_failed, peer_alive, run.rank, run.t_start);
}

void Heartbeat::stop() {
    stop_.store(true);
    if (t_.joinable()) t_.join();
}

void wait_for_row(const Run& run, const std::string& fin, int owner, int i) {
    const double w0 = now_s();
    while (access(fin.c_str(), F_OK) != 0) {
        struct stat sb;
        // (by now every rank that started in this attempt has removed the failure marker of an earlier one: a marker that is there is
        // this attempt's, or that of a rank that never started — dead either way; same rule as the watchdog's)
        if (peer_failed(run, owner)) DIE("rank %d failed before it finished volume %d", owner, i);
        const double now = now_s();
        if (stat(run.rf.alive(owner).c_str(), &sb) == 0) {
            if (now - (double)sb.st_mtime > 60.0) DIE("rank %d stopped responding (volume %d unfinished)", owner, i);
        } else if (now - w0 > 120.0 && access(fin.c_str(), F_OK) != 0) {
            DIE("rank %d is not running (no heartbeat; volume %d unfinished)", owner, i);
        }
        if (now - w0 > run.wait_limit) DIE("gave up waiting for volume %d of rank %d after %.0f s", i, owner, run.wait_limit);
        usleep(50 * 1000);
    }
}

// (same patience, and the same eye on failure markers, as for the rows)
void wait_for_partition_streams(const Run& run, const std::string& meta, int r, double w0) {
    while (access(meta.c_str(), F_OK) != 0) {
        if (peer_failed(run, r)) DIE("rank %d failed before it finished its partition streams", r);
        if (now_s() - w0 > run.wait_limit) DIE("gave up waiting for the partition streams of rank %d after %.0f s", r, run.wait_limit);
        usleep(20 * 1000);
    }
}
