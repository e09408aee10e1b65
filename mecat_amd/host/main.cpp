// main.cpp — mecat2pw: all-vs-all long-read overlapper, MI355X host driver (drop-in for the reference binary).
//
// Same process boundary as the reference: command line (options.cpp), wrk/vol<k> + wrk/fileindex.txt
// (volume.cpp), per-reference-volume result files wrk/r_<i>.working -> wrk/r_<i> with skip-if-finished resume, final
// `cat` in volume order (reference: mecat2pw/pw.cpp:14-85), `.can` lines (common/alignment.cpp:18-32) and `.m4` lines
// (mecat2pw/pw_impl.cpp:509-531).  What the reference does in its pthread workers (pw_impl.cpp:623-818) is done by three
// calls into libmecat_hip.so per (reference volume, query volume) grid cell: index build, seed_reads, align_candidates.
// Record assembly, the per-read m4 post-filter (std::sort + containment, pw_impl.cpp:539-610) and text output stay on
// the host (`-t` threads; the same option sizes the FASTA reader's thread pool).  There is no CPU fallback for the kernels: any failure aborts with the library's message.
//
// Additive, environment-only knobs:  MECAT_HIP_DEVICE=<n> (default 0),  MECAT_HIP_SLAB=<reads per seed call>,
// WORLD_SIZE / RANK / LOCAL_RANK (or MECAT_HIP_WORLD / MECAT_HIP_RANK): one process per GPU (see "Multi-GPU mode" in pw_run.h),
// MECAT_HIP_SHARD=rows|cells, MECAT_HIP_SHARD_CHUNK=<reads>, MECAT_HIP_RUN_ID=<token>, MECAT_HIP_COMM=file (test hook).
//
// This file: the run as a sequence of steps (main).  The parts: pw_run (the multi-process protocol), pw_row (one grid row: process_one_volume), pw_slabs (slab buffers and their hand-over
// to the writer thread), pw_format (what one read becomes in the output), pw_resident (volumes kept on the device), pw_common.
#include <errno.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>

#include "options.h"
#include "partition.h"
#include "pw_common.h"
#include "pw_resident.h"
#include "pw_row.h"
#include "pw_run.h"
#include "volume.h"

static std::string results_name(const char* wrk_dir, int vid, bool working) {
    std::string s(wrk_dir);
    if (s.empty() || s[s.size() - 1] != '/') s += '/';
    s += "r_" + std::to_string(vid);
    if (working) s += ".working";
    return s;
}

// r_<i> appended to (first: replacing) the output file, copied inside the kernel.  false = not an ordinary file (or the copy could
// not be made this way): the caller falls back to the reference's `cat`.
static bool merge_copy(const std::string& fin, const char* output, bool first) {
    struct stat so;
    const int have = lstat(output, &so);
    if (have == 0 && !S_ISREG(so.st_mode)) return false;
    if (have != 0 && errno != ENOENT) return false;
    if (have == 0 && first && unlink(output) != 0) return false;
    if (have == 0 && !first && so.st_nlink > 1) return false;
    const int in = open(fin.c_str(), O_RDONLY);
    if (in < 0) return false;
    const int out = open(output, O_WRONLY | O_CREAT | (first ? O_EXCL : 0), 0666);
    if (out < 0) { close(in); return false; }
    struct stat si;
    bool ok = fstat(in, &si) == 0 && lseek(out, 0, SEEK_END) >= 0;
    off_t left = ok ? si.st_size : 0;
    const off_t at0 = ok ? lseek(out, 0, SEEK_CUR) : 0;
    bool plain = false;
    while (ok && left > 0) {
        const ssize_t n = plain ? -1 : copy_file_range(in, NULL, out, NULL, (size_t)std::min<off_t>(left, (off_t)1 << 30), 0);
        if (n > 0) { left -= n; continue; }
        if (n == 0) break;
        // no copy_file_range between these two files (EXDEV, EINVAL, ENOSYS ...): plain read / write from where it stopped
        plain = true;
        static char buf[1 << 20];
        const ssize_t r = read(in, buf, sizeof(buf));
        if (r < 0) { ok = false; break; }
        if (r == 0) break;
        for (ssize_t w = 0; w < r;) {
            const ssize_t k = write(out, buf + w, (size_t)(r - w));
            if (k <= 0) { ok = false; break; }
            w += k;
        }
        left -= r;
    }
    ok = ok && left == 0;
    close(in);
    if (close(out) != 0) ok = false;
    if (!ok) {
        if (first) unlink(output);
        else if (truncate(output, at0) != 0) DIE("write error on '%s'", output);
    }
    return ok;
}

// The GPU context and the index-build scratch (two arrays of 8 bytes per base of a volume: hundreds of milliseconds to map
// at volume size) are set up on a second thread while the main thread parses the input.
struct GpuSetup {
    mhip_ctx* ctx = NULL;
    std::atomic<int> state{0};                       // 0 pending, 1 ready, -1 failed
    std::string error;
    std::thread t;
    void start(const Options& opt, int device);
    void join() { if (t.joinable()) t.join(); }
    mhip_ctx* wait_for_context();
    ~GpuSetup() { join(); }
};

void GpuSetup::start(const Options& opt, int device) {
    long long est_bases = 0;
    struct stat sb;
    FILE* f = fopen(opt.reads, "rb");
    if (f && fstat(fileno(f), &sb) == 0) {
        const int c0 = fgetc(f);
        est_bases = (long long)sb.st_size / (c0 == '@' ? 2 : 1);      // FASTQ carries a quality byte per base
    }
    if (f) fclose(f);
    est_bases = std::min(est_bases, (long long)kMaxVolumeBases + 64);
    if (getenv("MECAT_HIP_NO_RESERVE")) est_bases = 0;
    t = std::thread([this, device, est_bases]() {
        TraceTimer tt("ctx_create+reserve (background)");
        mhip_ctx* made = NULL;
        int rc = -1;
        for (int attempt = 0; attempt < 3 && rc != 0; ++attempt) {      // several processes opening a cold device at once can see a transient failure
            if (attempt) usleep(300 * 1000);
            rc = mhip_ctx_create(device, NULL, &made);
        }
        if (rc != 0) {
            error = mhip_last_error();
            state.store(-1);
            return;
        }
        ctx = made;
        state.store(1);
        if (est_bases > 0) (void)mhip_ctx_reserve_index(made, est_bases);      // best effort
    });
}

mhip_ctx* GpuSetup::wait_for_context() {
    TraceTimer tt("wait for ctx_create");
    // only the context is needed from here on; a reservation still in flight is waited for inside the library
    while (state.load() == 0) usleep(500);
    if (state.load() < 0) { join(); DIE("cannot use the GPU: %s", error.c_str()); }
    return ctx;
}

// rank 0 splits the input, lists the rows still to do and (multi-process) publishes both; the other ranks wait for that
static Split split_or_await(const Options& opt, const Run& run, GpuSetup& gpu, bool file_comm) {
    Split s;
    if (run.rank != 0) {
        await_split(run, opt.wrk_dir, &s);
        return s;
    }
    if (run.world > 1) unlink(run.rf.marker().c_str());
    for (int r = 0; run.world > 1 && r < run.world; ++r) unlink(partition_meta_name(opt.output, r).c_str());      // (no rank has started its partition streams yet)
    volume_set_async_dump(run.world == 1);       // other ranks read the volume files as soon as the run marker exists
    volume_set_device_packer([&gpu]() -> mhip_ctx* {      // (only used under MECAT_HIP_SPLIT=gpu)
        gpu.join();      // (the set-up thread still uses the context after it has published it)
        return gpu.state.load() == 1 ? gpu.ctx : NULL;
    });
    s.num_vols = split_raw_dataset(opt.reads, opt.wrk_dir, opt.num_threads);
    for (int i = 0; i < s.num_vols; ++i)
        if (access(results_name(opt.wrk_dir, i, false).c_str(), F_OK) != 0) s.todo.push_back(i);
    if (run.world > 1) {
        const char* se = getenv("MECAT_HIP_SHARD");
        s.cells = se ? !strcmp(se, "cells") : s.num_vols < run.world;
        if (s.cells && !file_comm) MCHK(mhip_comm_unique_id(s.comm_id));
        publish_split(run, s);
    }
    return s;
}

// MECAT_HIP_PARTITION=<batch_size>[,<min_read_size>[,<mapping_ratio>]] (additive): also write mecat2cns' partition files
// <output>.part<k> + <output>.partition_files (partition.h) — partition_candidates for -j 0, partition_m4records for
// -j 1 -g 1.  Records are taken straight from the result arrays: in a one-process run by the one writer, in a multi-process run by a
// writer per rank whose streams rank 0 merges at the end (partition.h: same bytes as the one-process files, no text parsed).  Only
// after a resume — finished rows' records are on disk as text alone — the merged text is partitioned.
struct PartitionOpts {
    long batch = 0;      // 0: no partition files
    int min_read = 0;
    double ratio = 0;
};
static PartitionOpts partition_options(const Options& opt) {
    PartitionOpts p;
    p.min_read = opt.tech == TECH_NANOPORE ? 2000 : 5000;      // mecat2cns defaults -l and -r, options.cpp:13-27
    p.ratio = opt.tech == TECH_NANOPORE ? 0.4 : 0.9;
    if (const char* pe = getenv("MECAT_HIP_PARTITION")) {
        if (opt.task == TASK_ALN && !opt.output_gapped_start_point)
            DIE("MECAT_HIP_PARTITION with -j 1 needs -g 1 (mecat2cns reads the gapped start points)");
        p.batch = atol(pe);
        if (const char* comma = strchr(pe, ',')) {
            p.min_read = atoi(comma + 1);
            if (const char* c2 = strchr(comma + 1, ',')) p.ratio = atof(c2 + 1);
        }
        if (p.batch <= 0) DIE("MECAT_HIP_PARTITION: batch size must be positive");
    }
    p.ratio = p.ratio - 0.02;                               // reads_correction_m4.cpp:79
    return p;
}

// rows mode: the static, cost-aware deal of the rows still to do (mhip_shard_deal_rows: row i costs num_vols - i cells; every rank
// derives it from the split marker's list alone)
static std::vector<int> deal_rows(const Run& run, const Split& s) {
    std::vector<int> row_owner((size_t)s.num_vols, 0);
    if (run.world <= 1 || s.cells) return row_owner;
    const int heaviest = mhip_shard_deal_rows(s.num_vols, s.todo.data(), (int)s.todo.size(), run.world, row_owner.data());
    if (heaviest < 0) DIE("cannot deal %d rows to %d ranks", (int)s.todo.size(), run.world);
    if (run.rank == 0 && getenv("MECAT_TRACE")) {
        long total = 0;
        for (int i : s.todo) total += s.num_vols - i;
        fprintf(stderr, "[trace] rows dealt: heaviest rank %d cells of %ld (mean %.2f)\n", heaviest, total, (double)total / run.world);
    }
    return row_owner;
}

// the grid rows of this rank.  rows: the owner of row i writes r_<i>.  cells: every rank writes the lines of its own reads to
// r_<i>.part<rank>, and once all parts are closed rank 0 strings them together into r_<i>.working -> r_<i> (the resume protocol sees
// only complete rows)
static void run_rows(const Options& opt, const Run& run, const Split& s, const std::vector<int>& row_owner, mhip_ctx* ctx, mhip_comm* comm,
                     const std::vector<std::string>& vn, PartitionWriter* pw, double part_ratio) {
    const int shard_chunk = std::max(1, env_int("MECAT_HIP_SHARD_CHUNK", NULL, MHIP_SHARD_CHUNK));
    for (int i = 0; i < s.num_vols; ++i) {
        if (std::find(s.todo.begin(), s.todo.end(), i) == s.todo.end()) {
            if (run.rank == 0) fprintf(stderr, "[main, %u] volume %d has been finished\n\n", __LINE__, i);
            continue;
        }
        if (!s.cells && run.world > 1 && row_owner[(size_t)i] != run.rank) continue;      // rows: dealt out by cost
        const std::string fin = results_name(opt.wrk_dir, i, false), wrk = results_name(opt.wrk_dir, i, true);
        const std::string mine = s.cells ? fin + ".part" + std::to_string(run.rank) : wrk;
        FILE* out = fopen(mine.c_str(), "w");
        if (!out) DIE("failed to open file '%s' with mode 'ios::out'", mine.c_str());
        if (pw) pw->set_row(i);
        process_one_volume(opt, ctx, i, vn, out, pw, part_ratio, comm, shard_chunk);
        if (fclose(out) != 0) DIE("write error!");
        if (s.cells) {
            MCHK(mhip_comm_barrier(comm));
            if (run.rank == 0) {
                TraceTimer tt("parts -> r_<i>");
                for (int r = 0; r < run.world; ++r) {
                    const std::string part = fin + ".part" + std::to_string(r);
                    if (!merge_copy(part, wrk.c_str(), r == 0)) DIE("cannot append '%s' to '%s'", part.c_str(), wrk.c_str());
                    unlink(part.c_str());
                }
            }
        }
        if (!s.cells || run.rank == 0)
            if (rename(wrk.c_str(), fin.c_str()) != 0) DIE("cannot rename %s", wrk.c_str());
    }
}

// merge_results, pw.cpp:34-46 (rank 0; in rows mode it waits for the rows of the other ranks, but not for a dead one)
static void merge_results(const Options& opt, const Run& run, const Split& s, const std::vector<int>& row_owner) {
    TraceTimer tt("merge_results");
    for (int i = 0; i < s.num_vols; ++i) {
        const std::string fin = results_name(opt.wrk_dir, i, false);
        if (run.world > 1 && !s.cells) wait_for_row(run, fin, row_owner[(size_t)i] >= 0 ? row_owner[(size_t)i] : 0, i);
        // The reference runs `cat r_<i> > output` / `>> output` through the shell (pw.cpp:34-46).  Same bytes here, copied inside the
        // kernel (copy_file_range: a reflink where the file system has one) when the output is, or is going to be, an ordinary file; an
        // existing output that is not a regular file (a FIFO, /dev/stdout) is written through by the shell as before.  The output never
        // shares an inode with r_<i> (a hard link would let a later `cat r_0 > output` of a resumed reference run truncate
        // both), and an old output is never written through: it is removed first, so a name that is a second link to some other file
        // cannot damage that file.  MECAT_HIP_MERGE=cat keeps the shell.
        if (!(getenv("MECAT_HIP_MERGE") && !strcmp(getenv("MECAT_HIP_MERGE"), "cat")) && merge_copy(fin, opt.output, i == 0)) continue;
        if (i == 0) {
            struct stat so;
            if (lstat(opt.output, &so) == 0 && S_ISREG(so.st_mode) && so.st_nlink > 1) unlink(opt.output);
        }
        const std::string cmd = std::string("cat ") + fin + (i == 0 ? " >" : " >> ") + opt.output;
        if (system(cmd.c_str()) != 0) DIE("'%s' failed", cmd.c_str());
    }
}

// rank 0: the partition files — from the records gathered on the way (pw; in a multi-process run merged with the other ranks' streams,
// which are complete when their meta files are there), or, after a resume, from the merged text
static void finish_partitions(const Options& opt, const Run& run, const PartitionOpts& part, PartitionWriter* pw) {
    if (pw) {
        TraceTimer tt("partition_files");
        pw->finish();
        delete pw;
        if (run.world > 1) {
            const double w0 = now_s();
            for (int r = 1; r < run.world; ++r) wait_for_partition_streams(run, partition_meta_name(opt.output, r), r, w0);
            partition_merge_ranks(opt.output, run.world, part.batch);
        }
    } else if (part.batch > 0) {
        TraceTimer tt("partition_files(text)");
        if (opt.task == TASK_SEED) partition_candidates_text(opt.output, part.batch, part.min_read, opt.num_threads);
        else partition_m4_text(opt.output, part.ratio, part.batch, part.min_read, opt.num_threads);
    }
}

// Rank 0's way out.  Everything this run owes the caller is on disk and closed.  What a plain `return` would still do — the HIP runtime's
// own teardown (code objects, queues, its threads) and the destructors of the statics — takes 40 - 80 ms and produces nothing: leave at
// once, after the two things that a skipped exit handler or destructor would have done: the volume file still being written on its
// thread (a resumed run whose rows were all finished has not waited for it anywhere), and the heartbeat thread, which removes its file.
[[noreturn]] static void leave(Heartbeat& beat) {
    volume_wait_pending();
    beat.stop();
    fflush(NULL);
    _exit(0);
}

int main(int argc, char* argv[]) {
    Options opt;
    if (parse_arguments(argc, argv, &opt)) {
        print_usage(argv[0]);
        return 1;
    }
    const Run run = run_from_env(opt.wrk_dir);
    GpuSetup gpu;
    gpu.start(opt, env_int("MECAT_HIP_DEVICE", run.world > 1 ? "LOCAL_RANK" : NULL, 0));
    Heartbeat beat;
    beat.start(run);
    const bool file_comm = getenv("MECAT_HIP_COMM") && !strcmp(getenv("MECAT_HIP_COMM"), "file");
    const Split split = split_or_await(opt, run, gpu, file_comm);
    const std::string idx_name = index_file_name(opt.wrk_dir);
    if (run.rank == 0) printf("%s\n", idx_name.c_str());
    const std::vector<std::string> vn = load_volume_names(idx_name);
    if ((int)vn.size() != split.num_vols) DIE("assertion 'num_vols == vn->num_vols' failed");

    mhip_ctx* ctx = gpu.wait_for_context();
    mhip_comm* comm = NULL;
    if (split.cells) {
        TraceTimer tt("comm_init");
        if (file_comm) MCHK(mhip_comm_init_hostfile(ctx, run.world, run.rank, opt.wrk_dir, run.rf.token.c_str(), &comm));
        else MCHK(mhip_comm_init(ctx, run.world, run.rank, split.comm_id, &comm));
        MCHK(mhip_comm_barrier(comm));
    }
    const PartitionOpts part = partition_options(opt);
    const std::vector<int> row_owner = deal_rows(run, split);
    PartitionWriter* pw = part.batch > 0 ? new PartitionWriter(opt.output, part.batch, part.min_read, run.world > 1 ? run.rank : -1) : NULL;
    if (pw && (int)split.todo.size() != split.num_vols) { pw->abandon(); delete pw; pw = NULL; }      // finished rows' records are only on disk (every rank sees the same list)
    run_rows(opt, run, split, row_owner, ctx, comm, vn, pw, part.ratio);
    if (comm) {
        MCHK(mhip_comm_barrier(comm));
        mhip_comm_destroy(comm);
    }
    gpu.join();
    {
        TraceTimer tt("ctx_destroy");
        resident_clear();
        mhip_ctx_destroy(ctx);
    }
    if (getenv("MECAT_TRACE")) fprintf(stderr, "[trace] main up to here     %.3f s\n", now_s() - run.t_start);
    if (run.rank != 0) {
        if (pw) { pw->finish(); delete pw; }      // this rank's record streams, complete (rank 0 merges them)
        return 0;
    }
    merge_results(opt, run, split, row_owner);
    finish_partitions(opt, run, part, pw);
    if (getenv("MECAT_TRACE")) fprintf(stderr, "[trace] main returns at    %.3f s\n", now_s() - run.t_start);
    leave(beat);
}
