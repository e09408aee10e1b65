// comm.hip — multi-GPU entry points of the C ABI (include/mecat_hip.h).
//
// The reference parallelises one grid cell (reference volume i x query volume j) over pthreads that pull chunks of 500
// query reads from a shared cursor (mecat2pw/pw_impl.cpp:612-621, 866-876).  Here the same chunks are dealt out statically
// to the P GPUs of a node — chunk c of query volume j belongs to rank (c + j) mod P — every rank seeds (and extends) the reads of
// its own chunks against its own copy of the index (rebuilt locally: recompute beats shipping up to 8.5 GB of positions over
// a 153 GB/s xGMI link), and the per-read candidate lists are exchanged in ONE all-gather per slab of reads:
//     counts first   ncclAllGather of one int32 per read
//     then payload   only the occupied 48-byte candidate_save records (about 22 of MAXC = 100 per read at config 2), as a
//                    grouped ncclSend / ncclRecv with every peer — xGMI is point to point, every pair of GPUs has its own link,
//                    so the all-gather-v is P - 1 direct transfers per rank in parallel, not a ring
// after which every rank holds the complete table in mhip_seed_reads' layout (rank 0 writes r_<i>, the file protocol is
// unchanged).  The extension results (32 bytes per candidate) travel the same way.
//
// RCCL is opened lazily (dlopen) by mhip_comm_init, so single-GPU runs never map the library.  mhip_comm_init_hostfile is a
// TEST HOOK: RCCL refuses two ranks on one device ("Duplicate GPU detected"), so the two-process tests on a one-GPU box
// exchange through files in a directory instead; same call sequence, same kernels, host-staged transport.
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "common.h"
#include "index_part.h"
#include "scan.h"

int mhip_seed_reads_chunked_dev(mhip_ctx* c, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid0, int chunk,
                                int nranks, int n, const mhip_params* P, void* d_out, void* d_out_counts);

namespace {

struct RcclApi {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
};

RcclApi* rccl() {
    static RcclApi api;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (api.handle) return &api;
    // a copy already mapped by the process (e.g. the one torch ships) is found by its SONAME; otherwise ROCm's
    const char* names[] = {getenv("MECAT_HIP_RCCL"), "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
    void* h = nullptr;
    for (const char* n : names) {
        if (!n || !*n) continue;
        h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (h) break;
    }
    if (!h) { mhip_set_error("cannot load RCCL (librccl.so.1): %s", dlerror()); return nullptr; }
#define SYM(f)                                                                         \
    api.f = (decltype(api.f))dlsym(h, "nccl" #f);                                       \
    if (!api.f) { mhip_set_error("RCCL symbol nccl" #f " missing"); dlclose(h); return nullptr; }
    SYM(GetUniqueId) SYM(CommInitRank) SYM(CommDestroy) SYM(AllGather) SYM(Send) SYM(Recv) SYM(GroupStart) SYM(GroupEnd) SYM(GetErrorString) SYM(CommCount)
#undef SYM
    api.handle = h;
    return &api;
}

#define NCHK(expr)                                                                                            \
    do {                                                                                                      \
        ncclResult_t r_ = (expr);                                                                             \
        if (r_ != ncclSuccess) { mhip_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, rccl()->GetErrorString(r_)); return -1; } \
    } while (0)

// ---- shard arithmetic: reads [rb, re) of a volume in chunks of `chunk`; chunk c belongs to rank (c + shift) mod P
struct Shard {
    int rb, re, chunk, shift, P;
    int cb() const { return rb / chunk; }
    int first_chunk(int rank) const {
        const int b = cb();
        return b + (((rank - (b + shift)) % P) + P) % P;
    }
    int rid0(int rank) const { return first_chunk(rank) * chunk; }
    int local_count(int rank) const {
        long n = 0;
        for (long c = first_chunk(rank); c * chunk < re; c += P) n += std::min<long>(re, (c + 1) * chunk) - c * chunk;
        return (int)n;
    }
};
__host__ __device__ inline int shard_rid(int rid0, int chunk, int P, int i) { return rid0 + (i / chunk) * chunk * P + i % chunk; }

}  // namespace

struct mhip_comm {
    mhip_ctx* ctx = nullptr;
    int nranks = 1, rank = 0;
    ncclComm_t nc = nullptr;
    // host-file transport (test hook)
    bool hostfile = false;
    // no transport at all (bench hook, mhip_comm_init_solo): this rank does its own share of every sharded call, its peers' contributions read
    // as zero bytes / zero counts — what one rank of P computes, alone on the device (bench.py --simulate-ranks)
    bool solo = false;
    int64_t bytes_sent = 0;                 // what this rank's contributions amount to on the links: its bytes to each of the P - 1 peers
    std::string dir, run_id;
    unsigned long seq = 0;
    // state of the last mhip_seed_reads_sharded call (consumed by mhip_align_sharded)
    Shard sh{0, 0, 1, 0, 1};
    int maxc = 0, n_pad = 0;
    std::vector<int64_t> totals;            // candidates per rank
    mhip_candidate* d_local = nullptr;      // [n_local][maxc]
    int32_t* d_local_cnt = nullptr;         // [n_local]
    int32_t* d_cnt_all = nullptr;           // [P][n_pad]
    uint32_t* d_pref = nullptr;             // [P][n_pad] exclusive prefix of d_cnt_all inside each rank
    mhip_candidate* d_all = nullptr;        // [re - rb][maxc]
    int32_t* d_all_cnt = nullptr;           // [re - rb]
    mhip_aln_result* d_all_res = nullptr;   // dense, read-major
    int64_t n_jobs_total = 0;
    int64_t bytes_received = 0;
    const char* xlabel = "xg_exchange";     // name the exchanges are timed under (HIP events on the stream while the context profiles)
    // mhip_index_build_auto: -1 undecided, 0 every rank rebuilds the table, 1 key-range shards + all-gather; the two times it measured
    int index_choice = -1;
    double index_ms[2] = {0.0, 0.0};
};

namespace {

// one block per rank: exclusive prefix of its counts, total to totals[rank]
__global__ __launch_bounds__(1024) void xg_prefix(const int32_t* __restrict__ cnt_all, int n_pad, uint32_t* __restrict__ pref, long long* __restrict__ totals) {
    const int r = blockIdx.x;
    const int32_t* __restrict__ cnt = cnt_all + (size_t)r * n_pad;
    uint32_t* __restrict__ row = pref + (size_t)r * n_pad;
    const unsigned int total = scan_array_1024<unsigned int>(n_pad, 0u, [&](long long i) { return (unsigned int)cnt[i]; }, [&](long long i, unsigned int p) { row[i] = p; });
    if (threadIdx.x == 0) totals[r] = (long long)total;
}

// this rank's occupied records, dense, local read-major
__global__ void xg_pack(const mhip_candidate* __restrict__ cands, const int32_t* __restrict__ cnt, const uint32_t* __restrict__ pref, int n_local,
                        int maxc, mhip_candidate* __restrict__ pack) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / (unsigned)maxc), k = (int)(t % (unsigned)maxc);
    if (i >= n_local || k >= cnt[i]) return;
    pack[(size_t)pref[i] + k] = cands[(size_t)i * maxc + k];
}

// dense rank-major records -> the read-major table of mhip_seed_reads
__global__ void xg_scatter(const mhip_candidate* __restrict__ dense, const int32_t* __restrict__ cnt_all, const uint32_t* __restrict__ pref,
                           const long long* __restrict__ displ, int n_pad, int maxc, int rb, int re, int chunk, int P, const int* __restrict__ rid0s,
                           mhip_candidate* __restrict__ all, int32_t* __restrict__ all_cnt) {
    const int r = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / (unsigned)maxc), k = (int)(t % (unsigned)maxc);
    if (i >= n_pad) return;
    const int rid = shard_rid(rid0s[r], chunk, P, i);
    if (rid >= re) return;
    const int c = cnt_all[(size_t)r * n_pad + i];
    if (k == 0) all_cnt[rid - rb] = c;
    if (k < c) all[(size_t)(rid - rb) * maxc + k] = dense[(size_t)displ[r] + pref[(size_t)r * n_pad + i] + k];
}

// jobs of this rank's reads, dense at pref[i] + k (the loop head of pairwise_mapping, pw_impl.cpp:674-686)
__global__ void xg_make_jobs(const mhip_candidate* __restrict__ cands, const int32_t* __restrict__ cnt, const uint32_t* __restrict__ pref, int n_local,
                             int maxc, int rid0, int chunk, int P, int ref_start_id, mhip_aln_job* __restrict__ jobs) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / (unsigned)maxc), k = (int)(t % (unsigned)maxc);
    if (i >= n_local || k >= cnt[i]) return;
    const mhip_candidate cd = cands[(size_t)i * maxc + k];
    mhip_aln_job jb;
    jb.qid_local = shard_rid(rid0, chunk, P, i);
    jb.sid_local = cd.readno - ref_start_id;
    jb.chain = cd.chain;
    int qstart = cd.loc2, sstart = cd.loc1;
    if (qstart && sstart) { qstart += MHIP_KMER_SIZE / 2; sstart += MHIP_KMER_SIZE / 2; }
    jb.qstart = qstart;
    jb.sstart = sstart;
    jobs[(size_t)pref[i] + k] = jb;
}

// exclusive scan of the read-major counts (one block)
__global__ __launch_bounds__(1024) void xg_read_first(const int32_t* __restrict__ counts, int n, uint32_t* __restrict__ first) {
    scan_array_1024<unsigned int>(n, 0u, [&](long long i) { return (unsigned int)counts[i]; }, [&](long long i, unsigned int p) { first[i] = p; });
}

// dense rank-major results -> dense read-major results
__global__ void xg_scatter_res(const mhip_aln_result* __restrict__ dense, const int32_t* __restrict__ cnt_all, const uint32_t* __restrict__ pref,
                               const long long* __restrict__ displ, int n_pad, int maxc, int rb, int re, int chunk, int P, const int* __restrict__ rid0s,
                               const uint32_t* __restrict__ first, mhip_aln_result* __restrict__ all) {
    const int r = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = (int)(t / (unsigned)maxc), k = (int)(t % (unsigned)maxc);
    if (i >= n_pad) return;
    const int rid = shard_rid(rid0s[r], chunk, P, i);
    if (rid >= re) return;
    if (k < cnt_all[(size_t)r * n_pad + i]) all[(size_t)first[rid - rb] + k] = dense[(size_t)displ[r] + pref[(size_t)r * n_pad + i] + k];
}

// ---- transport: every rank contributes bytes[rank] bytes at d_send; afterwards d_recv + displ[r] holds rank r's bytes on every rank
int allgatherv(mhip_comm* cm, const void* d_send, void* d_recv, const std::vector<size_t>& bytes, const std::vector<size_t>& displ) {
    mhip_ctx* c = cm->ctx;
    const int P = cm->nranks, me = cm->rank;
    if (bytes[me]) HIPCHK(hipMemcpyAsync((char*)d_recv + displ[me], d_send, bytes[me], hipMemcpyDeviceToDevice, c->stream));
    if (P == 1) return 0;
    for (int r = 0; r < P; ++r)
        if (r != me) cm->bytes_received += (int64_t)bytes[r];
    cm->bytes_sent += (int64_t)bytes[me] * (int64_t)(P - 1);
    if (cm->solo) {      // the peers' slots read as zeros (their sizes are whatever this rank believes them to be: zero counts -> zero bytes)
        for (int r = 0; r < P; ++r)
            if (r != me && bytes[r]) HIPCHK(hipMemsetAsync((char*)d_recv + displ[r], 0, bytes[r], c->stream));
        return 0;
    }
    LaunchTimer xt(c, cm->xlabel);
    if (!cm->hostfile) {
        RcclApi* R = rccl();
        if (!R) return -1;
        bool equal = true;
        for (int r = 0; r < P; ++r) equal = equal && bytes[r] == bytes[0] && displ[r] == (size_t)r * bytes[0];
        if (equal) {
            if (bytes[0]) NCHK(R->AllGather(d_send, d_recv, bytes[0], ncclInt8, cm->nc, c->stream));
            return 0;
        }
        NCHK(R->GroupStart());
        for (int r = 0; r < P; ++r) {
            if (r == me) continue;
            if (bytes[me]) NCHK(R->Send(d_send, bytes[me], ncclInt8, r, cm->nc, c->stream));
            if (bytes[r]) NCHK(R->Recv((char*)d_recv + displ[r], bytes[r], ncclInt8, r, cm->nc, c->stream));
        }
        NCHK(R->GroupEnd());
        return 0;
    }
    // host-file transport (test hook): one file per rank and exchange, written under a temporary name and renamed
    const unsigned long seq = cm->seq++;
    std::vector<char> h(std::max<size_t>(bytes[me], 1));
    if (bytes[me]) HIPCHK(hipMemcpyAsync(h.data(), d_send, bytes[me], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    auto name = [&](int r) { return cm->dir + "/xchg." + cm->run_id + "." + std::to_string(seq) + "." + std::to_string(r); };
    {
        const std::string tmp = name(me) + ".tmp";
        FILE* f = fopen(tmp.c_str(), "wb");
        if (!f || (bytes[me] && fwrite(h.data(), 1, bytes[me], f) != bytes[me]) || fclose(f) != 0) { mhip_set_error("cannot write %s", tmp.c_str()); return -1; }
        if (rename(tmp.c_str(), name(me).c_str()) != 0) { mhip_set_error("cannot rename %s", tmp.c_str()); return -1; }
    }
    for (int r = 0; r < P; ++r) {
        if (r == me) continue;
        const std::string fn = name(r);
        struct stat sb;
        long waited = 0;
        const long limit_ms = 1000L * (getenv("MECAT_HIP_COMM_TIMEOUT_S") ? atol(getenv("MECAT_HIP_COMM_TIMEOUT_S")) : 120L);
        while (stat(fn.c_str(), &sb) != 0) {
            usleep(2000);
            if ((waited += 2) > limit_ms) { mhip_set_error("rank %d never wrote %s (waited %ld s)", r, fn.c_str(), limit_ms / 1000); return -1; }
        }
        if ((size_t)sb.st_size != bytes[r]) { mhip_set_error("%s: %ld bytes, expected %zu", fn.c_str(), (long)sb.st_size, bytes[r]); return -1; }
        std::vector<char> g(std::max<size_t>(bytes[r], 1));
        FILE* f = fopen(fn.c_str(), "rb");
        if (!f || (bytes[r] && fread(g.data(), 1, bytes[r], f) != bytes[r])) { mhip_set_error("cannot read %s", fn.c_str()); if (f) fclose(f); return -1; }
        fclose(f);
        if (bytes[r]) HIPCHK(hipMemcpy((char*)d_recv + displ[r], g.data(), bytes[r], hipMemcpyHostToDevice));
    }
    // a rank may only remove its own file once every peer has read it: the file of exchange seq - 2 is certainly consumed
    if (seq >= 2) unlink((cm->dir + "/xchg." + cm->run_id + "." + std::to_string(seq - 2) + "." + std::to_string(me)).c_str());
    return 0;
}

// Failure is made collective before every payload exchange: each rank contributes one status word (0 = its local work of this
// step succeeded), and a step any rank failed fails on EVERY rank with the same return code — instead of one rank returning early
// while its peers sit in ncclAllGather / ncclSend / ncclRecv waiting for it.  `local_err` != 0 keeps the rank's own
// error text; the others name the rank that failed.
int agree(mhip_comm* cm, int local_err, const char* what) {
    mhip_ctx* c = cm->ctx;
    const int P = cm->nranks;
    if (P == 1) return local_err ? -1 : 0;
    int32_t* d;
    if (c->scratch("xg_status", sizeof(int32_t) * (size_t)(P + 1), (void**)&d)) {
        // no room for P + 1 words: this rank cannot even report; the peers' watchdogs (driver) or the transport's timeout end the step
        return -1;
    }
    const int32_t mine = local_err ? 1 : 0;
    if (hipMemcpyAsync(d + P, &mine, sizeof(mine), hipMemcpyHostToDevice, c->stream) != hipSuccess) return -1;
    std::vector<size_t> bytes((size_t)P, sizeof(int32_t)), displ((size_t)P);
    for (int r = 0; r < P; ++r) displ[(size_t)r] = sizeof(int32_t) * (size_t)r;
    std::string own = local_err ? mhip_last_error() : "";
    if (allgatherv(cm, d + P, d, bytes, displ)) return -1;
    std::vector<int32_t> st((size_t)P);
    if (hipMemcpyAsync(st.data(), d, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        mhip_set_error("%s: status exchange failed", what);
        return -1;
    }
    for (int r = 0; r < P; ++r)
        if (st[(size_t)r]) {
            if (local_err) mhip_set_error("%s", own.c_str());
            else mhip_set_error("%s: rank %d failed its part of the step; every rank stops", what, r);
            return -1;
        }
    return 0;
}

}  // namespace

extern "C" {

// the occupied entries of a candidate table, dense and read-major (what crosses the PCIe link for the text output: a list is
// ~22 of its 100 slots at config 2)
int mhip_pack_candidates_dev(mhip_ctx* c, const void* d_cands, const void* d_counts, int n_reads, int maxc, void* d_pack, int64_t* total) {
    HIPCHK(hipSetDevice(c->device));
    *total = 0;
    if (n_reads <= 0) return 0;
    uint32_t* d_pref;
    long long* d_tot;
    if (c->scratch("pk_pref", sizeof(uint32_t) * (size_t)n_reads, (void**)&d_pref)) return -1;
    if (c->scratch("pk_total", sizeof(long long), (void**)&d_tot)) return -1;
    LAUNCH(c, "xg_prefix", xg_prefix, 1, 1024, 0, (const int32_t*)d_counts, n_reads, d_pref, d_tot);
    const size_t nt = (size_t)n_reads * (size_t)maxc;
    LAUNCH(c, "xg_pack", xg_pack, (unsigned)((nt + 255) / 256), 256, 0, (const mhip_candidate*)d_cands, (const int32_t*)d_counts,
           (const uint32_t*)d_pref, n_reads, maxc, (mhip_candidate*)d_pack);
    long long t = 0;
    HIPCHK(hipMemcpyAsync(&t, d_tot, sizeof(t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *total = (int64_t)t;
    return 0;
}


int mhip_comm_unique_id(uint8_t id[MHIP_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == MHIP_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    RcclApi* R = rccl();
    if (!R) return -1;
    ncclUniqueId u;
    NCHK(R->GetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return 0;
}

int mhip_comm_init(mhip_ctx* ctx, int nranks, int rank, const uint8_t id[MHIP_COMM_ID_BYTES], mhip_comm** out) {
    *out = nullptr;
    if (nranks < 1 || rank < 0 || rank >= nranks) { mhip_set_error("bad rank %d of %d", rank, nranks); return -1; }
    HIPCHK(hipSetDevice(ctx->device));
    mhip_comm* cm = new mhip_comm();
    cm->ctx = ctx;
    cm->nranks = nranks;
    cm->rank = rank;
    if (nranks > 1) {
        RcclApi* R = rccl();
        if (!R) { delete cm; return -1; }
        ncclUniqueId u;
        memcpy(&u, id, sizeof(u));
        ncclResult_t r = R->CommInitRank(&cm->nc, nranks, u, rank);
        if (r != ncclSuccess) { mhip_set_error("ncclCommInitRank(rank %d of %d) failed: %s", rank, nranks, R->GetErrorString(r)); delete cm; return -1; }
    }
    // the status words of agree() exist from here on: reporting a failure never depends on an allocation made at the time of the failure
    void* d_status;
    if (ctx->scratch("xg_status", sizeof(int32_t) * (size_t)(nranks + 1), &d_status)) { mhip_comm_destroy(cm); return -1; }
    *out = cm;
    return 0;
}

int mhip_comm_init_hostfile(mhip_ctx* ctx, int nranks, int rank, const char* dir, const char* run_id, mhip_comm** out) {
    *out = nullptr;
    if (nranks < 1 || rank < 0 || rank >= nranks || !dir || !run_id) { mhip_set_error("bad host-file communicator arguments"); return -1; }
    mhip_comm* cm = new mhip_comm();
    cm->ctx = ctx;
    cm->nranks = nranks;
    cm->rank = rank;
    cm->hostfile = true;
    cm->dir = dir;
    cm->run_id = run_id;
    void* d_status;
    if (ctx->scratch("xg_status", sizeof(int32_t) * (size_t)(nranks + 1), &d_status)) { delete cm; return -1; }
    *out = cm;
    return 0;
}

// bench hook (bench.py --simulate-ranks): rank `rank` of `nranks` with NO transport — every sharded call does this rank's share of the
// work (its key range of the index, its chunks of the reads, the pack / scatter kernels of the exchanges) and moves nothing
int mhip_comm_init_solo(mhip_ctx* ctx, int nranks, int rank, mhip_comm** out) {
    *out = nullptr;
    if (nranks < 1 || rank < 0 || rank >= nranks) { mhip_set_error("bad solo communicator arguments"); return -1; }
    mhip_comm* cm = new mhip_comm();
    cm->ctx = ctx;
    cm->nranks = nranks;
    cm->rank = rank;
    cm->solo = true;
    void* d_status;
    if (ctx->scratch("xg_status", sizeof(int32_t) * (size_t)(nranks + 1), &d_status)) { delete cm; return -1; }
    *out = cm;
    return 0;
}
int64_t mhip_comm_bytes_sent(const mhip_comm* cm) { return cm->bytes_sent; }
// candidates (= extension jobs) of this rank's own reads in the slab of the last mhip_seed_reads_sharded call
int64_t mhip_comm_local_jobs(const mhip_comm* cm) { return cm->totals.empty() ? 0 : cm->totals[(size_t)cm->rank]; }

void mhip_comm_destroy(mhip_comm* cm) {
    if (!cm) return;
    if (cm->nc) {
        (void)hipSetDevice(cm->ctx->device);
        (void)hipStreamSynchronize(cm->ctx->stream);
        RcclApi* R = rccl();
        if (R) (void)R->CommDestroy(cm->nc);
    }
    // (host-file transport: the files of the last two exchanges stay behind — a peer may still be reading them)
    delete cm;
}

// RCCL smoke test on one device: loads the library, creates a one-rank communicator on the context's device and runs the two
// transport forms of allgatherv (ncclAllGather; grouped ncclSend / ncclRecv, here to the rank itself) on the context's stream.
int mhip_comm_selftest(mhip_ctx* c) {
    HIPCHK(hipSetDevice(c->device));
    RcclApi* R = rccl();
    if (!R) return -1;
    ncclUniqueId u;
    NCHK(R->GetUniqueId(&u));
    ncclComm_t nc = nullptr;
    NCHK(R->CommInitRank(&nc, 1, u, 0));
    uint32_t* d;
    if (c->scratch("xg_selftest", 4 * 1024 * 3, (void**)&d)) return -1;
    std::vector<uint32_t> h(1024);
    for (int i = 0; i < 1024; ++i) h[(size_t)i] = 0x9e3779b9u * (uint32_t)(i + 1);
    HIPCHK(hipMemcpyAsync(d, h.data(), 4096, hipMemcpyHostToDevice, c->stream));
    NCHK(R->AllGather(d, d + 1024, 4096, ncclInt8, nc, c->stream));
    NCHK(R->GroupStart());
    NCHK(R->Send(d, 4096, ncclInt8, 0, nc, c->stream));
    NCHK(R->Recv(d + 2048, 4096, ncclInt8, 0, nc, c->stream));
    NCHK(R->GroupEnd());
    std::vector<uint32_t> g(2048);
    HIPCHK(hipMemcpyAsync(g.data(), d + 1024, 8192, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)R->CommDestroy(nc);
    for (int i = 0; i < 1024; ++i)
        if (g[(size_t)i] != h[(size_t)i] || g[(size_t)i + 1024] != h[(size_t)i]) { mhip_set_error("RCCL self test: wrong data at word %d", i); return -1; }
    return 0;
}

// what the communicator really is: transport 0 = RCCL, 1 = host files (test hook); rccl_ranks = ncclCommCount of the RCCL
// communicator (0 with the host-file transport) — a bench line that claims N GPUs shows that RCCL saw N ranks
int mhip_comm_info(const mhip_comm* cm, int* transport, int* rccl_ranks) {
    if (transport) *transport = cm->solo ? 2 : (cm->hostfile ? 1 : 0);
    if (rccl_ranks) {
        *rccl_ranks = 0;
        if (!cm->hostfile && !cm->solo && cm->nc) {
            RcclApi* R = rccl();
            if (!R) return -1;
            int n = 0;
            NCHK(R->CommCount(cm->nc, &n));
            *rccl_ranks = n;
        }
    }
    return 0;
}
int mhip_comm_rank(const mhip_comm* cm) { return cm->rank; }
int mhip_comm_nranks(const mhip_comm* cm) { return cm->nranks; }
int64_t mhip_comm_bytes_received(const mhip_comm* cm) { return cm->bytes_received; }

int mhip_comm_barrier(mhip_comm* cm) {
    mhip_ctx* c = cm->ctx;
    HIPCHK(hipSetDevice(c->device));
    char* d;
    if (c->scratch("xg_barrier", 64 * (size_t)(cm->nranks + 1), (void**)&d)) return -1;
    std::vector<size_t> bytes((size_t)cm->nranks, 64), displ((size_t)cm->nranks);
    for (int r = 0; r < cm->nranks; ++r) displ[(size_t)r] = 64 * (size_t)(r + 1);
    if (allgatherv(cm, d, d, bytes, displ)) return -1;      // (self copy d -> d + 64 (rank + 1): disjoint)
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int mhip_shard_local_count(int rid_begin, int rid_end, int chunk, int cell_shift, int rank, int nranks) {
    if (chunk < 1 || nranks < 1 || rid_begin % chunk != 0) return -1;
    const Shard s{rid_begin, rid_end, chunk, cell_shift, nranks};
    return s.local_count(rank);
}
int mhip_shard_first_read(int rid_begin, int rid_end, int chunk, int cell_shift, int rank, int nranks) {
    if (chunk < 1 || nranks < 1 || rid_begin % chunk != 0) return -1;
    const Shard s{rid_begin, rid_end, chunk, cell_shift, nranks};
    return s.rid0(rank);
}

// rows mode: longest-processing-time deal of the grid rows still to do (mecat_hip.h)
int mhip_shard_deal_rows(int num_vols, const int* todo, int ntodo, int nranks, int* owner) {
    if (num_vols < 0 || ntodo < 0 || nranks < 1 || (ntodo && !todo) || (num_vols && !owner)) return -1;
    for (int i = 0; i < num_vols; ++i) owner[i] = -1;
    std::vector<int> rows;
    for (int k = 0; k < ntodo; ++k) {
        if (todo[k] < 0 || todo[k] >= num_vols || owner[todo[k]] == -2) return -1;
        owner[todo[k]] = -2;
        rows.push_back(todo[k]);
    }
    std::sort(rows.begin(), rows.end());                  // ascending row = descending cost
    std::vector<long> load((size_t)nranks, 0), cells((size_t)nranks, 0);
    for (int i : rows) {
        int best = 0;
        for (int r = 1; r < nranks; ++r)
            if (load[(size_t)r] < load[(size_t)best]) best = r;
        owner[i] = best;
        load[(size_t)best] += 4L * (num_vols - i) + 1;   // cells of the row + a quarter cell for its index build
        cells[(size_t)best] += num_vols - i;
    }
    long mx = 0;
    for (long v : cells) mx = std::max(mx, v);
    return (int)mx;
}

// d_cands[n_local][maxc], d_counts[n_local]: this rank's reads of the shard (local index i = read rid0 + (i / chunk) * chunk * P + i % chunk).
// d_all_cands[(rid_end - rid_begin)][maxc], d_all_counts[rid_end - rid_begin]: the complete table, on every rank.
int mhip_allgather_candidates(mhip_comm* cm, const void* d_cands, const void* d_counts, int rid_begin, int rid_end, int chunk, int cell_shift,
                              int maxc, void* d_all_cands, void* d_all_counts) {
    mhip_ctx* c = cm->ctx;
    HIPCHK(hipSetDevice(c->device));
    const int P = cm->nranks, me = cm->rank;
    if (chunk < 1 || rid_begin % chunk != 0 || rid_end < rid_begin || maxc < 1) { mhip_set_error("bad shard [%d,%d) chunk %d", rid_begin, rid_end, chunk); return -1; }
    const Shard sh{rid_begin, rid_end, chunk, cell_shift, P};
    std::vector<int> nloc((size_t)P), rid0s((size_t)P);
    int n_pad = 1;
    for (int r = 0; r < P; ++r) { nloc[(size_t)r] = sh.local_count(r); rid0s[(size_t)r] = sh.rid0(r); n_pad = std::max(n_pad, nloc[(size_t)r]); }
    const int n_local = nloc[(size_t)me];
    cm->sh = sh;
    cm->maxc = maxc;
    cm->n_pad = n_pad;
    int32_t *d_pad = nullptr, *d_cnt_all = nullptr;
    uint32_t* d_pref = nullptr;
    long long* d_tot = nullptr;      // [P] totals, [P] displacements
    int* d_rid0 = nullptr;
    {
        const int lerr = c->scratch("xg_cntpad", sizeof(int32_t) * (size_t)n_pad, (void**)&d_pad) ||
                         c->scratch("xg_cntall", sizeof(int32_t) * (size_t)n_pad * P, (void**)&d_cnt_all) ||
                         c->scratch("xg_pref", sizeof(uint32_t) * (size_t)n_pad * P, (void**)&d_pref) ||
                         c->scratch("xg_tot", sizeof(long long) * 2 * (size_t)P, (void**)&d_tot) ||
                         c->scratch("xg_rid0", sizeof(int) * (size_t)P, (void**)&d_rid0);
        if (agree(cm, lerr, "mhip_allgather_candidates (count buffers)")) return -1;
    }
    HIPCHK(hipMemsetAsync(d_pad, 0, sizeof(int32_t) * (size_t)n_pad, c->stream));
    if (n_local) HIPCHK(hipMemcpyAsync(d_pad, d_counts, sizeof(int32_t) * (size_t)n_local, hipMemcpyDeviceToDevice, c->stream));
    // 1. counts
    {
        std::vector<size_t> bytes((size_t)P, sizeof(int32_t) * (size_t)n_pad), displ((size_t)P);
        for (int r = 0; r < P; ++r) displ[(size_t)r] = bytes[0] * (size_t)r;
        if (allgatherv(cm, d_pad, d_cnt_all, bytes, displ)) return -1;
    }
    LAUNCH(c, "xg_prefix", xg_prefix, P, 1024, 0, (const int32_t*)d_cnt_all, n_pad, d_pref, d_tot);
    std::vector<long long> tot((size_t)P);
    HIPCHK(hipMemcpyAsync(tot.data(), d_tot, sizeof(long long) * (size_t)P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    cm->totals.assign(tot.begin(), tot.end());
    std::vector<long long> displ_rec((size_t)P);
    long long total = 0;
    for (int r = 0; r < P; ++r) { displ_rec[(size_t)r] = total; total += tot[(size_t)r]; }
    cm->n_jobs_total = total;
    HIPCHK(hipMemcpyAsync(d_tot + P, displ_rec.data(), sizeof(long long) * (size_t)P, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_rid0, rid0s.data(), sizeof(int) * (size_t)P, hipMemcpyHostToDevice, c->stream));
    // 2. payload: only the occupied records
    // (every rank holds the same totals[]: size limits are checked on all of them, so that all ranks fail alike)
    for (int r = 0; r < P; ++r)
        if (tot[(size_t)r] > 0x7fffffffLL) { mhip_set_error("rank %d holds %lld candidates of this slab (limit 2^31 - 1): use smaller slabs", r, tot[(size_t)r]); return -1; }
    mhip_candidate *d_pack = nullptr, *d_dense = nullptr;
    {
        const int lerr = c->scratch("xg_pack", sizeof(mhip_candidate) * (size_t)std::max<long long>(tot[(size_t)me], 1), (void**)&d_pack) ||
                         c->scratch("xg_dense", sizeof(mhip_candidate) * (size_t)std::max<long long>(total, 1), (void**)&d_dense);
        if (agree(cm, lerr, "mhip_allgather_candidates (payload buffers)")) return -1;
    }
    if (n_local) {
        const size_t nt = (size_t)n_local * (size_t)maxc;
        LAUNCH(c, "xg_pack", xg_pack, (unsigned)((nt + 255) / 256), 256, 0, (const mhip_candidate*)d_cands, (const int32_t*)d_counts,
               (const uint32_t*)(d_pref + (size_t)me * n_pad), n_local, maxc, d_pack);
    }
    {
        std::vector<size_t> bytes((size_t)P), displ((size_t)P);
        for (int r = 0; r < P; ++r) { bytes[(size_t)r] = sizeof(mhip_candidate) * (size_t)tot[(size_t)r]; displ[(size_t)r] = sizeof(mhip_candidate) * (size_t)displ_rec[(size_t)r]; }
        if (allgatherv(cm, d_pack, d_dense, bytes, displ)) return -1;
    }
    // 3. back into the read-major table
    const int n = rid_end - rid_begin;
    if (n > 0) {
        HIPCHK(hipMemsetAsync(d_all_counts, 0, sizeof(int32_t) * (size_t)n, c->stream));
        const size_t nt = (size_t)n_pad * (size_t)maxc;
        LAUNCH(c, "xg_scatter", xg_scatter, dim3((unsigned)((nt + 255) / 256), (unsigned)P), 256, 0, (const mhip_candidate*)d_dense,
               (const int32_t*)d_cnt_all, (const uint32_t*)d_pref, (const long long*)(d_tot + P), n_pad, maxc, rid_begin, rid_end, chunk, P,
               (const int*)d_rid0, (mhip_candidate*)d_all_cands, (int32_t*)d_all_counts);
    }
    HIPCHK(hipGetLastError());
    cm->d_cnt_all = d_cnt_all;
    cm->d_pref = d_pref;
    return 0;
}

int mhip_seed_reads_sharded(mhip_comm* cm, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                            int chunk, int cell_shift, const mhip_params* P, mhip_candidate* out, int32_t* out_counts) {
    mhip_ctx* c = cm->ctx;
    HIPCHK(hipSetDevice(c->device));
    if (rid_begin < 0 || rid_end > reads->num_reads || rid_begin > rid_end || chunk < 1 || rid_begin % chunk != 0) {
        mhip_set_error("bad sharded read range [%d,%d) chunk %d", rid_begin, rid_end, chunk);
        return -1;
    }
    const int n = rid_end - rid_begin;
    if (n == 0) return 0;
    const Shard sh{rid_begin, rid_end, chunk, cell_shift, cm->nranks};
    const int n_local = sh.local_count(cm->rank);
    {
        int lerr = c->scratch("xg_local", sizeof(mhip_candidate) * (size_t)std::max(n_local, 1) * (size_t)P->maxc, (void**)&cm->d_local) ||
                   c->scratch("xg_localcnt", sizeof(int32_t) * (size_t)std::max(n_local, 1), (void**)&cm->d_local_cnt) ||
                   c->scratch("xg_all", sizeof(mhip_candidate) * (size_t)n * (size_t)P->maxc, (void**)&cm->d_all) ||
                   c->scratch("xg_allcnt", sizeof(int32_t) * (size_t)n, (void**)&cm->d_all_cnt);
        if (!lerr && n_local) lerr = mhip_seed_reads_chunked_dev(c, idx, ref, reads, sh.rid0(cm->rank), chunk, cm->nranks, n_local, P, cm->d_local, cm->d_local_cnt);
        if (!lerr && hipStreamSynchronize(c->stream) != hipSuccess) { mhip_set_error("seeding of this rank's reads failed on the device"); lerr = 1; }
        if (agree(cm, lerr, "mhip_seed_reads_sharded")) return -1;      // a rank whose seeding failed takes every rank out before the exchange
    }
    if (mhip_allgather_candidates(cm, cm->d_local, cm->d_local_cnt, rid_begin, rid_end, chunk, cell_shift, P->maxc, cm->d_all, cm->d_all_cnt)) return -1;
    if (out_counts) HIPCHK(hipMemcpyAsync(out_counts, cm->d_all_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (out) HIPCHK(hipMemcpyAsync(out, cm->d_all, sizeof(mhip_candidate) * (size_t)n * (size_t)P->maxc, hipMemcpyDeviceToHost, c->stream));
    if (out || out_counts) HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int mhip_align_sharded(mhip_comm* cm, const mhip_volume* ref, const mhip_volume* reads, int tech, int min_align_size, mhip_aln_result* out,
                       int64_t* num_jobs) {
    mhip_ctx* c = cm->ctx;
    HIPCHK(hipSetDevice(c->device));
    const int P = cm->nranks, me = cm->rank;
    const Shard& sh = cm->sh;
    const int n = sh.re - sh.rb;
    if (num_jobs) *num_jobs = cm->n_jobs_total;
    if (n <= 0 || cm->totals.empty()) return 0;
    const int n_local = sh.local_count(me), maxc = cm->maxc, n_pad = cm->n_pad;
    const long long mine = cm->totals[(size_t)me], total = cm->n_jobs_total;
    mhip_aln_job* d_jobs = nullptr;
    mhip_aln_result *d_res = nullptr, *d_dense = nullptr;
    {
        int lerr = c->scratch("xg_jobs", sizeof(mhip_aln_job) * (size_t)std::max<long long>(mine, 1), (void**)&d_jobs) ||
                   c->scratch("xg_res", sizeof(mhip_aln_result) * (size_t)std::max<long long>(mine, 1), (void**)&d_res) ||
                   c->scratch("xg_resdense", sizeof(mhip_aln_result) * (size_t)std::max<long long>(total, 1), (void**)&d_dense) ||
                   c->scratch("xg_resall", sizeof(mhip_aln_result) * (size_t)std::max<long long>(total, 1), (void**)&cm->d_all_res);
        if (!lerr && mine) {      // (mine <= 2^31 - 1: checked on every rank's total in mhip_allgather_candidates)
            const size_t nt = (size_t)n_local * (size_t)maxc;
            LAUNCH(c, "xg_make_jobs", xg_make_jobs, (unsigned)((nt + 255) / 256), 256, 0, (const mhip_candidate*)cm->d_local, (const int32_t*)cm->d_local_cnt,
                   (const uint32_t*)(cm->d_pref + (size_t)me * n_pad), n_local, maxc, sh.rid0(me), sh.chunk, P, ref->start_read_id, d_jobs);
            lerr = tech == 1 ? mhip_xalign_candidates_dev(c, ref, reads, d_jobs, (int)mine, min_align_size, d_res)
                             : mhip_align_candidates_dev(c, ref, reads, d_jobs, (int)mine, min_align_size, d_res);
            if (!lerr && hipStreamSynchronize(c->stream) != hipSuccess) { mhip_set_error("extension of this rank's candidates failed on the device"); lerr = 1; }
        }
        if (agree(cm, lerr, "mhip_align_sharded")) return -1;
    }
    std::vector<size_t> bytes((size_t)P), displ((size_t)P);
    std::vector<long long> displ_rec((size_t)P);
    long long acc = 0;
    for (int r = 0; r < P; ++r) {
        displ_rec[(size_t)r] = acc;
        bytes[(size_t)r] = sizeof(mhip_aln_result) * (size_t)cm->totals[(size_t)r];
        displ[(size_t)r] = sizeof(mhip_aln_result) * (size_t)acc;
        acc += cm->totals[(size_t)r];
    }
    if (allgatherv(cm, d_res, d_dense, bytes, displ)) return -1;
    long long* d_tot;
    int* d_rid0;
    uint32_t* d_first;
    if (c->scratch("xg_tot", sizeof(long long) * 2 * (size_t)P, (void**)&d_tot)) return -1;       // [P + r] = displacements, still valid
    if (c->scratch("xg_rid0", sizeof(int) * (size_t)P, (void**)&d_rid0)) return -1;
    if (c->scratch("xg_first", sizeof(uint32_t) * (size_t)n, (void**)&d_first)) return -1;
    LAUNCH(c, "xg_read_first", xg_read_first, 1, 1024, 0, (const int32_t*)cm->d_all_cnt, n, d_first);
    const size_t nt = (size_t)n_pad * (size_t)maxc;
    LAUNCH(c, "xg_scatter_res", xg_scatter_res, dim3((unsigned)((nt + 255) / 256), (unsigned)P), 256, 0, (const mhip_aln_result*)d_dense,
           (const int32_t*)cm->d_cnt_all, (const uint32_t*)cm->d_pref, (const long long*)(d_tot + P), n_pad, maxc, sh.rb, sh.re, sh.chunk, P,
           (const int*)d_rid0, (const uint32_t*)d_first, cm->d_all_res);
    HIPCHK(hipGetLastError());
    if (out && total) {
        HIPCHK(hipMemcpyAsync(out, cm->d_all_res, sizeof(mhip_aln_result) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int mhip_sharded_tables(mhip_comm* cm, void** d_cands, void** d_counts, void** d_results, int64_t* num_jobs) {
    if (d_cands) *d_cands = cm->d_all;
    if (d_counts) *d_counts = cm->d_all_cnt;
    if (d_results) *d_results = cm->d_all_res;
    if (num_jobs) *num_jobs = cm->n_jobs_total;
    return 0;
}

}  // extern "C"

namespace {
// after the slices of a sharded table have been gathered: bucket boundaries (and the .x of the bucket records) are relative to
// their rank's first kept position; add each rank's base.  ranges[r] = first k-mer id of rank r (ranges[P] = 4^13), base[r] = kept
// positions in front of rank r.
__global__ void xg_index_rebase(uint32_t* __restrict__ starts, uint4* __restrict__ recs, const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ base, int P) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= NKMER) return;
    int r = 0;
    while (r + 1 < P && ranges[r + 1] <= id) ++r;
    const uint32_t b = base[r];
    starts[id] += b;
    if (recs) recs[id].x += b;
}
}  // namespace

extern "C" {

// The look-up table of one volume built by all ranks together (SURVEY.md §8e said "replicate by recomputation"; with the build at
// 23 ms the replicated build is the non-scaling term of a sharded grid cell: VERDICT r02).  The 512 level-1 bins of the partition
// build (index_part.hip) are cut into P contiguous key ranges of about equal occupancy (every rank derives the same cut from its own
// first volume walk, no exchange); a rank runs both volume walks but partitions, fills and keeps only its own range; then
//     counts    one int64 per rank (kept positions), same transport as the candidate exchange
//     payload   positions (4 B each), the slices of starts[] and of the bucket records — each rank's bytes to every peer directly
// and every rank holds the complete table of mhip_index_build (slots[] are recomputed locally from the positions: one streaming
// pass instead of 2 more bytes per position over the links).  Per rank at config 2 and P = 8: 4.1 GB of positions + 1.2 GB of
// table slices received, against a rebuild that is 23 ms whatever P is.
int mhip_index_build_sharded(mhip_comm* cm, const mhip_volume* v, mhip_index** out) {
    struct Label { mhip_comm* c; Label(mhip_comm* c_) : c(c_) { c->xlabel = "xg_exchange_index"; } ~Label() { c->xlabel = "xg_exchange"; } } label_guard(cm);
    mhip_ctx* c = cm->ctx;
    *out = nullptr;
    HIPCHK(hipSetDevice(c->device));
    const int P = cm->nranks, me = cm->rank;
    if (P == 1) return mhip_index_build(c, v, out);
    // 1. the cut (identical on every rank: same volume, same walk)
    IxpSlice cnt;
    cnt.count_only = true;
    int lerr = index_build_partitioned(c, v, MAX_BUCKET, 0, IXP_NB1, &cnt);
    if (agree(cm, lerr, "mhip_index_build_sharded (first walk)")) return -1;
    std::vector<int> lo((size_t)P + 1, IXP_NB1);
    {
        const uint64_t total = cnt.bin_total[IXP_NB1];
        int b = 0;
        lo[0] = 0;
        for (int r = 1; r < P; ++r) {
            const uint64_t want = total * (uint64_t)r / (uint64_t)P;
            while (b < IXP_NB1 && (uint64_t)cnt.bin_total[(size_t)b] < want) ++b;
            lo[(size_t)r] = b;
        }
        lo[(size_t)P] = IXP_NB1;
    }
    const int bin_lo = lo[(size_t)me], bin_hi = lo[(size_t)me + 1], nb = bin_hi - bin_lo;
    const size_t ids_mine = (size_t)nb * IXP_IDS_PER_BIN;
    // 2. this rank's slice, into scratch
    IxpSlice sl;
    struct Cx { mhip_ctx* c; } cx{c};
    sl.user = &cx;
    const int segs = (v->num_bases + 2000 - 1) / 2000;
    sl.cut_step = ((segs + 7) / 8) * 2000;
    sl.alloc = [](IxpSlice* s, size_t kept) -> int {
        mhip_ctx* c = ((Cx*)s->user)->c;
        if (c->scratch("xi_offsets", sizeof(int32_t) * (kept + 64), (void**)&s->d_offsets)) return -1;
        if (c->scratch("xi_slots", sizeof(uint16_t) * (kept + 64), (void**)&s->d_slots)) return -1;      // (written by the fill, not exchanged)
        return 0;
    };
    uint4* d_recs_slice = nullptr;
    lerr = c->scratch("xi_starts", sizeof(uint32_t) * (ids_mine + 1), (void**)&sl.d_starts) ||
           c->scratch("xi_recs", sizeof(uint4) * std::max<size_t>(ids_mine, 1), (void**)&d_recs_slice);
    if (!lerr) {
        sl.d_recs = d_recs_slice;
        // (the slice's recs pointer is fixed before the build: the alloc callback only adds the arrays sized by the kept count)
        if (nb > 0) lerr = index_build_partitioned(c, v, MAX_BUCKET, bin_lo, bin_hi, &sl);
        else sl.num_kept = 0;
    }
    if (agree(cm, lerr, "mhip_index_build_sharded (slice build)")) return -1;
    // 3. counts
    long long* d_k;
    if (c->scratch("xi_kept", sizeof(long long) * (size_t)(P + 1), (void**)&d_k)) lerr = 1;
    if (agree(cm, lerr, "mhip_index_build_sharded (count buffers)")) return -1;
    const long long mine = (long long)sl.num_kept;
    lerr = hipMemcpyAsync(d_k + P, &mine, sizeof(mine), hipMemcpyHostToDevice, c->stream) != hipSuccess;
    if (lerr) mhip_set_error("sharded index: cannot upload the kept count");
    if (agree(cm, lerr, "mhip_index_build_sharded (kept counts)")) return -1;
    {
        std::vector<size_t> bytes((size_t)P, sizeof(long long)), displ((size_t)P);
        for (int r = 0; r < P; ++r) displ[(size_t)r] = sizeof(long long) * (size_t)r;
        if (allgatherv(cm, d_k + P, d_k, bytes, displ)) return -1;
    }
    std::vector<long long> kept((size_t)P);
    HIPCHK(hipMemcpyAsync(kept.data(), d_k, sizeof(long long) * (size_t)P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> base((size_t)P + 1, 0u), ranges((size_t)P + 1);
    long long total = 0;
    for (int r = 0; r < P; ++r) { base[(size_t)r] = (uint32_t)total; total += kept[(size_t)r]; ranges[(size_t)r] = (uint32_t)lo[(size_t)r] * IXP_IDS_PER_BIN; }
    base[(size_t)P] = (uint32_t)total;
    ranges[(size_t)P] = NKMER;
    if (total > 0x7fffffffLL) { mhip_set_error("sharded index: %lld kept positions", total); return -1; }      // (the same on every rank)
    // 4. the table, complete on every rank
    mhip_index* idx = new mhip_index();
    struct IdxGuard { mhip_index* p; ~IdxGuard() { if (p) mhip_index_free(p); } } guard{idx};      // freed on every path that does not hand it out
    idx->device = c->device;
    idx->num_bases = v->num_bases;
    idx->max_bucket = MAX_BUCKET;
    idx->num_kmers = total;
    idx->cut_step = sl.cut_step;
    lerr = dev_alloc_recycled(c->device, sizeof(uint32_t) * ((size_t)NKMER + 1), (void**)&idx->d_starts, &idx->cap_starts) ||
           dev_alloc_recycled(c->device, sizeof(int32_t) * ((size_t)total + 64), (void**)&idx->d_offsets, &idx->cap_offsets) ||
           dev_alloc_recycled(c->device, sizeof(uint4) * (size_t)NKMER, (void**)&idx->d_recs, &idx->cap_recs);
    uint32_t* d_tab = nullptr;
    if (!lerr) lerr = c->scratch("xi_tab", sizeof(uint32_t) * 2 * (size_t)(P + 1), (void**)&d_tab);
    // the two small host tables go up before the status exchange, so that a failed copy is a reported failure of this rank and not an
    // early return with the peers inside the payload exchange
    if (!lerr && (hipMemcpyAsync(d_tab, ranges.data(), sizeof(uint32_t) * (size_t)(P + 1), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                  hipMemcpyAsync(d_tab + (P + 1), base.data(), sizeof(uint32_t) * (size_t)(P + 1), hipMemcpyHostToDevice, c->stream) != hipSuccess)) {
        mhip_set_error("sharded index: cannot upload the range table");
        lerr = 1;
    }
    if (agree(cm, lerr, "mhip_index_build_sharded (table arrays)")) return -1;
    {
        std::vector<size_t> bytes((size_t)P), displ((size_t)P);
        for (int r = 0; r < P; ++r) { bytes[(size_t)r] = sizeof(int32_t) * (size_t)kept[(size_t)r]; displ[(size_t)r] = sizeof(int32_t) * (size_t)base[(size_t)r]; }
        if (allgatherv(cm, sl.d_offsets, idx->d_offsets, bytes, displ)) return -1;
        for (int r = 0; r < P; ++r) {
            const size_t ids = (size_t)(lo[(size_t)r + 1] - lo[(size_t)r]) * IXP_IDS_PER_BIN;
            bytes[(size_t)r] = sizeof(uint32_t) * ids;
            displ[(size_t)r] = sizeof(uint32_t) * (size_t)ranges[(size_t)r];
        }
        if (allgatherv(cm, sl.d_starts, idx->d_starts, bytes, displ)) return -1;
        for (int r = 0; r < P; ++r) { bytes[(size_t)r] *= 4; displ[(size_t)r] *= 4; }      // 16-byte records
        if (allgatherv(cm, d_recs_slice, idx->d_recs, bytes, displ)) return -1;
    }
    // (nothing is exchanged from here on: a local failure ends this rank's call; its peers learn of it at the next agree())
    LAUNCH(c, "xg_index_rebase", xg_index_rebase, NKMER / 256, 256, 0, idx->d_starts, idx->d_recs, (const uint32_t*)d_tab, (const uint32_t*)(d_tab + (P + 1)), P);
    HIPCHK(hipMemcpyAsync(idx->d_starts + NKMER, d_tab + (P + 1) + P, sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    if (index_add_slots(c, idx)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));      // (the host tables above go out of scope)
    guard.p = nullptr;
    *out = idx;
    return 0;
}

// The table of a volume, built the faster of the two ways — every rank for itself (mhip_index_build) or together
// (mhip_index_build_sharded).  Which one wins depends on what the links of the node at hand deliver (DESIGN.md §5 priced it at an assumed
// 55 GB/s per xGMI link and put the break-even at four ranks; nobody has measured it on more than one GPU: VERDICT r04), so the first
// call on a communicator measures: both builds once to warm their buffers up, both again timed (barrier to barrier, the slowest rank's
// time counts), the faster one is kept for this and every later call.  MECAT_HIP_INDEX_SHARD=0 / 1 decides without measuring.
// ms[0] / ms[1] = the replicated / sharded times the decision rests on (0 when it was not measured); *sharded = what was used.
int mhip_index_build_auto(mhip_comm* cm, const mhip_volume* v, mhip_index** out, double ms[2], int* sharded) {
    mhip_ctx* c = cm->ctx;
    *out = nullptr;
    if (cm->index_choice < 0) {
        if (const char* e = getenv("MECAT_HIP_INDEX_SHARD")) cm->index_choice = atoi(e) != 0 && cm->nranks > 1;
        else if (cm->nranks == 1) cm->index_choice = 0;
    }
    if (cm->index_choice < 0) {
        double t[2] = {0.0, 0.0};
        mhip_index* keep[2] = {nullptr, nullptr};
        struct KeepGuard {      // an error return frees what was built so far
            mhip_index** k; bool armed = true;
            ~KeepGuard() { if (armed) for (int i = 0; i < 2; ++i) if (k[i]) { mhip_index_free(k[i]); k[i] = nullptr; } }
        } keep_guard{keep};
        for (int pass = 0; pass < 2; ++pass)
            for (int how = 0; how < 2; ++how) {
                if (keep[how]) { mhip_index_free(keep[how]); keep[how] = nullptr; }
                if (mhip_comm_barrier(cm)) return -1;
                const auto t0 = std::chrono::steady_clock::now();
                const int rc = how ? mhip_index_build_sharded(cm, v, &keep[how]) : mhip_index_build(c, v, &keep[how]);
                if (agree(cm, rc, "mhip_index_build_auto")) return -1;      // (ends with every rank's stream drained)
                t[how] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        // the slowest rank's times, the same on every rank: one exchange of two doubles per rank
        const int P = cm->nranks;
        double* d;
        if (c->scratch("xg_auto", sizeof(double) * 2 * (size_t)(P + 1), (void**)&d)) return -1;
        HIPCHK(hipMemcpyAsync(d + 2 * P, t, sizeof(t), hipMemcpyHostToDevice, c->stream));
        std::vector<size_t> bytes((size_t)P, sizeof(t)), displ((size_t)P);
        for (int r = 0; r < P; ++r) displ[(size_t)r] = sizeof(t) * (size_t)r;
        if (allgatherv(cm, d + 2 * P, d, bytes, displ)) return -1;
        std::vector<double> all((size_t)(2 * P));
        HIPCHK(hipMemcpyAsync(all.data(), d, sizeof(double) * 2 * (size_t)P, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int r = 0; r < P; ++r) { cm->index_ms[0] = std::max(cm->index_ms[0], all[(size_t)(2 * r)]); cm->index_ms[1] = std::max(cm->index_ms[1], all[(size_t)(2 * r + 1)]); }
        cm->index_choice = cm->index_ms[1] < cm->index_ms[0] ? 1 : 0;
        if (getenv("MECAT_TRACE") && cm->rank == 0)
            fprintf(stderr, "[mecat_hip] index build over %d ranks: every rank for itself %.1f ms, key-range shards + all-gather %.1f ms -> %s\n", P,
                    cm->index_ms[0], cm->index_ms[1], cm->index_choice ? "sharded" : "replicated");
        keep_guard.armed = false;
        mhip_index_free(keep[1 - cm->index_choice]);
        *out = keep[cm->index_choice];
    } else {
        if (cm->index_choice ? mhip_index_build_sharded(cm, v, out) : mhip_index_build(c, v, out)) return -1;
    }
    if (ms) { ms[0] = cm->index_ms[0]; ms[1] = cm->index_ms[1]; }
    if (sharded) *sharded = cm->index_choice;
    return 0;
}

}  // extern "C"
