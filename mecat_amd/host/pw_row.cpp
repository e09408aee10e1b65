// pw_row.cpp — one grid row of mecat2pw: reference volume `svid` against the query volumes svid .. V - 1 (process_one_volume).  What the
// reference does in its pthread workers (pw_impl.cpp:623-818) is done per cell by calls into libmecat_hip.so — index build, seeding,
// extension — slab by slab; a second thread (pw_slabs.h) turns each slab into text (pw_format.h) and writes it.
#include "pw_row.h"

#include <algorithm>

#include "partition.h"
#include "pw_common.h"
#include "pw_format.h"
#include "pw_resident.h"
#include "pw_slabs.h"

struct LibPin {
    static int lock(void* p, size_t bytes) { return mhip_host_register(p, bytes); }
    static void unlock(void* p) { mhip_host_unregister(p); }
};
typedef SlabBuf<LibPin> Slab;

struct RowRun {
    const Options& opt;
    mhip_ctx* ctx;
    const int svid;
    const std::vector<std::string>& vn;
    FILE* out;
    PartitionWriter* pw;
    const double part_ratio;
    mhip_comm* comm;      // NULL: this process computes the whole row
    const int shard_chunk;
    mhip_params P;
    int nt;               // formatting threads
    HostVolume ref_own;   // the reference volume: host tables, device copy, index
    const HostVolume* ref = NULL;
    bool ref_cached = false;
    mhip_volume* dref = NULL;
    mhip_index* idx = NULL;
    int slab = 0;         // reads per slab (shrinking: see open_row)
    bool shrinking = false;
    std::thread prealloc;
    double shown[ST_N] = {0, 0, 0, 0, 0, 0, 0, 0};      // the clocks at the last trace line
    SlabQueue<Slab> q;
    RowRun(const Options& o, mhip_ctx* c, int sv, const std::vector<std::string>& names, FILE* f, PartitionWriter* w, double ratio, mhip_comm* cm, int chunk);
};

struct Cell {             // one query volume of the row
    int vid = 0;
    HostVolume store;     // (only a volume that is not kept resident lives here)
    const HostVolume* rd = NULL;
    mhip_volume* dreads = NULL;
    bool cached = true;
    // one process: the resident candidate table of the current super-slab, reads [first, first + reads) of the volume
    void *d_cands = NULL, *d_counts = NULL;
    int first = 0, reads = 0, super_reads = 0;
};

static int slab_len(const RowRun& R, int rb, int end) {
    const int left = end - rb;
    if (!R.shrinking) return std::min(R.slab, left);
    int s2 = std::max(2000, (int)(0.7 * left));
    if (left - s2 < 2000) s2 = left;
    return std::min(s2, left);
}

// the writer thread's work on one slab: the text of its reads, by nt threads over equal read ranges, written in read order
static void write_slab(RowRun& R, Slab& B, double* clk) {
    const int nt = R.nt, nr = B.nr;
    // cells mode: every rank holds the slab's complete tables (the all-gather of the candidate lists and results) and formats
    // and writes the reads of its OWN chunks — chunk c of query volume vid belongs to rank (c + vid) mod P — into its own part
    // of r_<i>; rank 0 strings the parts together (main).  The line order of r_<i> is then "by rank" instead of "by read": the
    // multiset of lines is the contract, the reference's own order depends on its thread timing.
    const int c_rank = R.comm ? mhip_comm_rank(R.comm) : 0, c_world = R.comm ? mhip_comm_nranks(R.comm) : 1;
    const bool seed_only = R.opt.task == TASK_SEED;
    const CellReads T = {B.rd->offs.data(), B.rd->start_read_id, R.ref->offs.data(), R.ref->start_read_id};
    std::vector<std::string> text((size_t)nt);
    std::vector<std::vector<CanRec>> crec(R.pw && seed_only ? (size_t)nt : 0);
    std::vector<std::vector<M4Rec>> mrec(R.pw && !seed_only ? (size_t)nt : 0);
    {
        StageClock sc(&clk[ST_FORMAT]);
        run_threads(nt, [&](int t) {
            const int lo = (int)((long long)nr * t / nt), hi = (int)((long long)nr * (t + 1) / nt);
            M4Scratch scratch;
            for (int r = lo; r < hi; ++r) {
                if (c_world > 1 && ((B.rb + r) / R.shard_chunk + B.vid) % c_world != c_rank) continue;
                const size_t c0 = B.packed ? B.jfirst[(size_t)r] : (size_t)r * R.P.maxc;
                const int n = B.counts[(size_t)r];
                if (seed_only) format_can_read(T, B.rb + r, B.cands.data() + c0, n, text[(size_t)t], R.pw ? &crec[(size_t)t] : NULL);
                else format_m4_read(T, B.rb + r, B.cands.data() + c0, B.res.data() + B.jfirst[(size_t)r], n, R.opt.output_gapped_start_point != 0, scratch,
                                    text[(size_t)t], R.pw ? &mrec[(size_t)t] : NULL);
            }
        });
    }
    StageClock sc(&clk[seed_only ? ST_FORMAT : ST_WRITE]);      // (`-j 0` books its writing with the formatting)
    for (const std::string& o : text)
        if (!o.empty() && fwrite(o.data(), 1, o.size(), R.out) != o.size()) DIE("write error!");
    // the same lines, in the same order, as records (no text round trip)
    for (const std::vector<CanRec>& v : crec) R.pw->add(v.data(), v.size());
    for (const std::vector<M4Rec>& v : mrec) R.pw->add_m4(v.data(), v.size(), R.part_ratio);
}

RowRun::RowRun(const Options& o, mhip_ctx* c, int sv, const std::vector<std::string>& names, FILE* f, PartitionWriter* w, double ratio, mhip_comm* cm, int chunk)
    : opt(o), ctx(c), svid(sv), vn(names), out(f), pw(w), part_ratio(ratio), comm(cm), shard_chunk(chunk),
      nt(std::max(1, std::min(o.num_threads, 64))), q([this](Slab& B, double* clk) { write_slab(*this, B, clk); }) {
    mhip_params_default(&P, opt.tech);
    P.maxc = opt.num_candidates;
    P.min_align_size = opt.min_align_size;
    P.min_kmer_match = opt.min_kmer_match;
}

// the reference volume, the slab policy, and the slab buffers made on a thread of their own
static void open_row(RowRun& R) {
    R.dref = resident_get(R.ctx, R.vn, R.svid, &R.ref, &R.ref_own, &R.ref_cached);
    const bool ont_aln = R.opt.tech == TECH_NANOPORE && R.opt.task == TASK_ALN;
    const char* slab_env = getenv("MECAT_HIP_SLAB");
    // 20 000 reads per slab; nanopore extension: 60 000 — an X-drop call ends with the tail of its longest units (the waves pull units,
    // longest first, from one cursor: the last ones run on a chip that is emptying), so fewer, larger calls: 2 per config-5 cell instead
    // of 6.  (The second launch that used to end every call — rounds 1-3, the first reason for this size — is gone since round 4.)
    R.slab = slab_env ? std::max(1, atoi(slab_env)) : (ont_aln ? 60000 : 20000);
    if (R.comm) R.slab = std::max(R.shard_chunk, R.slab - R.slab % R.shard_chunk);      // slabs start on chunk boundaries
    // One process, PacBio gates: slabs of SHRINKING size — 70 % of the reads that are left, down to 2 000.  Formatting a slab takes a third
    // of the time its extension takes, so slab s is always written out before slab s + 1 comes off the GPU and only the LAST slab's
    // formatting is exposed at the end of the volume: the smaller it is the better, while every slab costs a fixed few milliseconds on
    // the device (the second extension launch for the handed-over units, the tails of the launches, the copies): 70 000 / 21 000 /
    // 6 300 / 2 700 reads at config 2 instead of five slabs of 20 000.  MECAT_HIP_SLAB keeps a fixed size.
    R.shrinking = !slab_env && !R.comm && !ont_aln;
    // page-locking ~100 MB per slab buffer takes 30-60 ms each: done on a second thread while the volume goes up and is indexed
    R.prealloc = std::thread([&R]() {
        const size_t rows = (size_t)std::max(1, slab_len(R, 0, std::max(R.ref->num_reads, 1)));      // (other query volumes of the row are no larger; buffers grow when one is)
        for (Slab& B : R.q.slabs) {
            B.cands.resize(R.comm ? rows * (size_t)R.P.maxc : rows * 32);       // packed lists in a one-process run (grown when a slab holds more)
            B.counts.resize(rows);
            if (R.opt.task != TASK_SEED) B.res.resize(rows * 32);       // (grown when a slab holds more candidates)
        }
    });
}

static void build_index(RowRun& R) {
    {
        ScopedTimer t("create_ref_index");
        // cells mode: the ranks either build the table together, each the buckets of its own k-mer key range, and gather positions and
        // table slices (mhip_index_build_sharded) — a replicated rebuild is the part of a sharded cell that does not shrink with the
        // number of GPUs — or every rank rebuilds it for itself (with few ranks the 4.7 GB of positions over one or two xGMI links can
        // cost more than the rebuild).  The first table of a run is built both ways, timed, and the faster way is kept
        // (mhip_index_build_auto; MECAT_HIP_INDEX_SHARD=0 / 1 decides without measuring).
        if (R.comm) MCHK(mhip_index_build_auto(R.comm, R.dref, &R.idx, NULL, NULL));
        else MCHK(mhip_index_build(R.ctx, R.dref, &R.idx));
    }
    printf("number of kmers: %lld\n", (long long)mhip_index_num_kmers(R.idx));
    R.prealloc.join();
}

static void get_query_volume(RowRun& R, Cell& C) {
    C.rd = R.ref;
    C.dreads = R.dref;
    C.cached = true;
    if (C.vid != R.svid) C.dreads = resident_get(R.ctx, R.vn, C.vid, &C.rd, &C.store, &C.cached);
}

// candidate_detect aborts on a read of MAX_SEQ_SIZE bases or more (pw_impl.cpp:743-746); pairwise_mapping would
// overrun its MAX_SEQ_SIZE buffers there.  Same limit, same message, for both tasks.
static void check_read_sizes(const HostVolume& rd) {
    for (int r = 0; r < rd.num_reads; ++r)
        if (rd.offs[(size_t)r].size >= MHIP_MAX_SEQ_SIZE) {
            printf("rsize = %d\t%d\n", rd.offs[(size_t)r].size, MHIP_MAX_SEQ_SIZE);
            fflush(stdout);
            abort();
        }
}

// One process: the candidate lists of the whole cell are made in one go and stay in HBM; a slab is then job assembly and
// extension on the device plus the copies the text needs (a seeding call per slab cost 5 x 17 ms instead of 59 at config 2,
// and the host-side job assembly kept the GPU waiting).  With a communicator the sharded calls do all of this.
// The resident table is [reads][MAXC] records of 48 bytes: a volume of short reads at a large -n would not fit (2 M reads at
// -n 1024: 100 GB), so the cell is seeded in super-slabs — a whole number of slabs whose table stays inside a budget taken from
// the free device memory (a quarter of it, at most 32 GB; MECAT_HIP_CELL_MB overrides) — one super-slab = the whole cell whenever
// it fits (config 2: 0.48 GB).
static void plan_super_slabs(RowRun& R, Cell& C) {
    C.super_reads = C.rd->num_reads;
    if (R.comm) return;
    size_t free_b = 0, total_b = 0;
    { StageClock sc(&R.q.gpu[ST_MEMQ]); MCHK(mhip_ctx_mem_info(R.ctx, &free_b, &total_b)); }
    size_t budget = std::min<size_t>(free_b / 4, (size_t)32 << 30);
    if (const char* e = getenv("MECAT_HIP_CELL_MB")) budget = (size_t)std::max(1L, atol(e)) << 20;
    const size_t per_read = sizeof(mhip_candidate) * (size_t)R.P.maxc + sizeof(int32_t);
    const size_t fit = R.shrinking ? std::max<size_t>(2000, budget / per_read) : std::max<size_t>(1, budget / per_read / (size_t)R.slab) * (size_t)R.slab;
    C.super_reads = (int)std::min<size_t>((size_t)std::max(C.rd->num_reads, 1), fit);
}

// seeds the super-slab that starts at read `first` into the resident table
static void seed_super_slab(RowRun& R, Cell& C, int first) {
    StageClock sc(&R.q.gpu[ST_SEED]);
    const size_t rows = (size_t)std::min(C.super_reads, C.rd->num_reads);
    C.first = first;
    C.reads = std::min(C.super_reads, C.rd->num_reads - first);
    MCHK(mhip_ctx_buffer(R.ctx, "cell_cands", sizeof(mhip_candidate) * rows * R.P.maxc, &C.d_cands));
    MCHK(mhip_ctx_buffer(R.ctx, "cell_counts", sizeof(int32_t) * rows, &C.d_counts));
    MCHK(mhip_seed_reads_dev(R.ctx, R.idx, R.dref, C.dreads, first, first + C.reads, &R.P, C.d_cands, C.d_counts));
    MCHK(mhip_ctx_sync(R.ctx));
}

static void count_prefix_sums(Slab& B) {
    B.jfirst.assign((size_t)B.nr + 1, 0);
    for (int r = 0; r < B.nr; ++r) B.jfirst[(size_t)r + 1] = B.jfirst[(size_t)r] + (size_t)B.counts[(size_t)r];
}

// one process: the counts, and the occupied entries of the lists packed on the device (a list is ~22 of its 100 slots)
static void fill_slab_from_table(RowRun& R, const Cell& C, Slab& B) {
    StageClock sc(&R.q.gpu[ST_WRITE]);      // (copies: booked with the writing)
    const int cb = B.rb - C.first, nr = B.nr;      // the slab inside the resident table
    MCHK(mhip_download(R.ctx, B.counts.data(), (const int32_t*)C.d_counts + cb, sizeof(int32_t) * (size_t)nr));
    count_prefix_sums(B);
    void* d_pack = NULL;
    int64_t total = 0;
    MCHK(mhip_ctx_buffer(R.ctx, "slab_pack", sizeof(mhip_candidate) * (size_t)nr * R.P.maxc, &d_pack));
    MCHK(mhip_pack_candidates_dev(R.ctx, (const mhip_candidate*)C.d_cands + (size_t)cb * R.P.maxc, (const int32_t*)C.d_counts + cb, nr, R.P.maxc, d_pack,
                                  &total));
    if ((size_t)total != B.jfirst[(size_t)nr]) DIE("%lld packed candidates for %zu counted", (long long)total, B.jfirst[(size_t)nr]);
    B.cands.resize((size_t)total);
    MCHK(mhip_download(R.ctx, B.cands.data(), d_pack, sizeof(mhip_candidate) * (size_t)total));
}

static void fill_slab_sharded(RowRun& R, const Cell& C, Slab& B) {
    StageClock sc(&R.q.gpu[ST_SEED]);
    MCHK(mhip_seed_reads_sharded(R.comm, R.idx, R.dref, C.dreads, B.rb, B.rb + B.nr, R.shard_chunk, C.vid, &R.P, B.cands.data(), B.counts.data()));
}

// pairwise_mapping, pw_impl.cpp:674-700, with the jobs made on the device from the lists that are there
static void extend_from_table(RowRun& R, const Cell& C, Slab& B) {
    const int cb = B.rb - C.first, nr = B.nr;
    { StageClock sc(&R.q.gpu[ST_PIN]); B.res.resize(B.jfirst[(size_t)nr]); }
    void *d_jobs = NULL, *d_res = NULL;
    int nj = 0;
    {
        StageClock sc(&R.q.gpu[ST_JOBS]);
        MCHK(mhip_ctx_buffer(R.ctx, "slab_jobs", sizeof(mhip_aln_job) * (size_t)nr * R.P.maxc, &d_jobs));
        MCHK(mhip_jobs_from_candidates_dev(R.ctx, (const mhip_candidate*)C.d_cands + (size_t)cb * R.P.maxc, (const int32_t*)C.d_counts + cb, nr, R.P.maxc,
                                           B.rb, 1, R.ref->start_read_id, 0, 1, d_jobs, &nj));
        if ((size_t)nj != B.jfirst[(size_t)nr]) DIE("%d jobs for %zu candidates", nj, B.jfirst[(size_t)nr]);
    }
    StageClock sc(&R.q.gpu[ST_EXTEND]);
    MCHK(mhip_ctx_buffer(R.ctx, "slab_results", sizeof(mhip_aln_result) * (size_t)std::max(nj, 1), &d_res));
    // aligner by technology (pw_impl.cpp:638-644): DiffAligner (dw) for PacBio, XdropAligner for nanopore
    if (R.opt.tech == TECH_NANOPORE) MCHK(mhip_xalign_candidates_dev(R.ctx, R.dref, C.dreads, d_jobs, nj, R.P.min_align_size, d_res));
    else MCHK(mhip_align_candidates_dev(R.ctx, R.dref, C.dreads, d_jobs, nj, R.P.min_align_size, d_res));
    MCHK(mhip_download(R.ctx, B.res.data(), d_res, sizeof(mhip_aln_result) * (size_t)nj));
}

// pairwise_mapping, pw_impl.cpp:674-700, sharded: the jobs of the gathered lists are assembled here, every rank extends its own
static void extend_sharded(RowRun& R, const Cell& C, Slab& B) {
    const int nr = B.nr, nt = R.nt;
    {
        StageClock sc(&R.q.gpu[ST_JOBS]);
        count_prefix_sums(B);
        B.jobs.resize(B.jfirst[(size_t)nr]);
        run_threads(nt, [&](int t) {
            const int lo = (int)((long long)nr * t / nt), hi = (int)((long long)nr * (t + 1) / nt);
            for (int r = lo; r < hi; ++r) {
                size_t jn = B.jfirst[(size_t)r];
                for (int k = 0; k < B.counts[(size_t)r]; ++k) B.jobs[jn++] = job_of_candidate(B.cands[(size_t)r * R.P.maxc + k], B.rb + r, R.ref->start_read_id);
            }
        });
        B.res.resize(B.jobs.size());
    }
    StageClock sc(&R.q.gpu[ST_EXTEND]);
    int64_t nj = 0;
    MCHK(mhip_align_sharded(R.comm, R.dref, C.dreads, R.opt.tech == TECH_NANOPORE ? 1 : 0, R.P.min_align_size, B.res.data(), &nj));
    if ((size_t)nj != B.jobs.size()) DIE("sharded extension returned %lld results for %zu candidates", (long long)nj, B.jobs.size());
}

// the slabs of a cell, each seeded (or taken from the resident table), extended and handed to the writer
static void fill_slabs(RowRun& R, Cell& C) {
    const int num_reads = C.rd->num_reads;
    bool first_of_cell = true;
    for (int rb = 0, step = 0; rb < num_reads; rb += step) {
        // (a slab never straddles two super-slabs of the resident table: it ends where the super-slab that holds its first read ends)
        const int super_end = R.comm ? num_reads : std::min(num_reads, (rb / C.super_reads + 1) * C.super_reads);
        step = slab_len(R, rb, super_end);
        Slab& B = R.q.acquire();                  // the buffers of slab sno - 2 must have been written out
        B.rb = rb;
        B.nr = step;
        B.packed = !R.comm;
        B.rd = C.rd;
        B.vid = C.vid;
        if (!R.comm && (first_of_cell || rb >= C.first + C.reads)) seed_super_slab(R, C, rb);
        first_of_cell = false;
        {
            StageClock sc(&R.q.gpu[ST_PIN]);
            if (R.comm) B.cands.resize((size_t)B.nr * R.P.maxc);
            B.counts.resize((size_t)B.nr);
        }
        if (R.comm) fill_slab_sharded(R, C, B);
        else fill_slab_from_table(R, C, B);
        if (R.opt.task != TASK_SEED) {
            if (R.comm) extend_sharded(R, C, B);
            else extend_from_table(R, C, B);
        }
        if (R.q.filled_so_far() == 0) volume_release_input();      // every scratch array of the volume exists by now
        R.q.filled();
    }
}

// MECAT_TRACE: what the clocks gathered since the last line (formatting of this cell's tail shows up in the next line); vid -1 = what
// the writer still did after the last cell
static void trace_stages(RowRun& R, int vid) {
    if (!getenv("MECAT_TRACE")) return;
    double st[ST_N], d[ST_N];
    R.q.snapshot(st);
    for (int k = 0; k < ST_N; ++k) d[k] = st[k] - R.shown[k];
    if (vid >= 0)
        fprintf(stderr, "[trace] volume %d stages: seed %.3f s, jobs %.3f s, extend %.3f s, format %.3f s, write + copies %.3f s, page-locked buffers %.3f s, slab buffer waits %.3f s, memory query %.3f s\n",
                vid, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
    else if (d[ST_FORMAT] > 0.0005 || d[ST_WRITE] > 0.0005)
        fprintf(stderr, "[trace] volume -1 stages: seed %.3f s, jobs %.3f s, extend %.3f s, format %.3f s, write + copies %.3f s, page-locked buffers %.3f s\n",
                d[0], d[1], d[2], d[3], d[4], d[5]);
    for (int k = 0; k < ST_N; ++k) R.shown[k] = st[k];
}

static void run_cell(RowRun& R, int vid) {
    char info[64];
    snprintf(info, sizeof(info), "process volume %d", vid);
    ScopedTimer t(info);
    fprintf(stderr, "[process_one_volume, %u] processing %s\n\n", __LINE__, R.vn[vid].c_str());
    Cell C;
    C.vid = vid;
    get_query_volume(R, C);
    check_read_sizes(*C.rd);
    plan_super_slabs(R, C);
    fill_slabs(R, C);
    if (!C.cached) R.q.drain();      // this cell's query volume goes away with the cell: its slabs have to be written out first
    trace_stages(R, vid);
    if (C.dreads != R.dref && !C.cached) mhip_volume_free(C.dreads);
}

static void close_row(RowRun& R) {
    R.q.close();
    trace_stages(R, -1);
    mhip_index_free(R.idx);
    if (!R.ref_cached) mhip_volume_free(R.dref);
    volume_wait_pending();       // the volume's file is written from `ref`'s buffers
}

void process_one_volume(const Options& opt, mhip_ctx* ctx, int svid, const std::vector<std::string>& vn, FILE* out, PartitionWriter* pw,
                        double part_ratio, mhip_comm* comm, int shard_chunk) {
    RowRun R(opt, ctx, svid, vn, out, pw, part_ratio, comm, shard_chunk);
    open_row(R);
    build_index(R);
    for (int vid = svid; vid < (int)vn.size(); ++vid) run_cell(R, vid);
    close_row(R);
}
