/*
 * mecat_hip.h — C ABI of libmecat_hip.so: the MI355X (gfx950) implementation of mecat2pw's hot path.
 *
 * This is the drop-in boundary.  MECAT has no plugin/FFI layer; the hot path sits behind three
 * function seams inside the mecat2pw binary, and each entry point below replaces one of them (reference file:line,
 * relative to /root/reference/src/):
 *
 *   mhip_index_build      <- create_ref_index / destroy_ref_index      common/lookup_table.h:13-17, lookup_table.cpp:63
 *   mhip_seed_reads       <- seeding + get_candidates, both strands     mecat2pw/pw_impl.cpp:241, :288, loop at :752-765
 *   mhip_align_candidates <- GapAligner::go + accessors (DiffAligner)   common/gapalign.h:4-25, diff_gapalign.cpp:294,
 *                                                                       called at mecat2pw/pw_impl.cpp:688-697
 *   mhip_xalign_candidates<- GapAligner::go + accessors (XdropAligner)  common/xdrop_gapalign.cpp:359 (nanopore, -x 1)
 *   mhip_volume_upload    <- load_volume's in-memory volume_t           common/split_database.h:18-24, split_database.cpp:155
 *   mhip_params           <- the file-static tuning values              mecat2pw/pw_impl.cpp:18-26, set at :838-851
 *
 * Conventions (mirroring the reference where it has any): plain C types only; opaque handles with explicit *_free;
 * every call returns 0 on success and non-zero on failure with the message in mhip_last_error() (the reference
 * abort()s instead — the host driver maps non-zero to abort-with-message).  Handles are immutable after creation and
 * may be shared by host threads; a context (one HIP stream + scratch) must not be used by two threads at once.
 * There is NO CPU fallback: every entry point fails if no gfx950 device is usable.
 *
 * INTEGRATION.md shows the binding a MECAT maintainer would add to call these from pw_impl.cpp.
 */
#ifndef MECAT_HIP_H
#define MECAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHIP_ABI_VERSION 1
#define MHIP_KMER_SIZE 13          /* pw_impl.cpp:20 */
#define MHIP_MAX_SEQ_SIZE 500000   /* common/defs.h:202 */

typedef struct mhip_ctx mhip_ctx;        /* device + stream + scratch arena */
typedef struct mhip_volume mhip_volume;  /* device-resident 2-bit volume (volume_t) */
typedef struct mhip_index mhip_index;    /* device-resident k-mer index (ref_index) */

typedef struct { int32_t offset, size; } mhip_offset_t;      /* offset_t, split_database.h:9-11 */

/* candidate_save, mecat2pw/pw_impl.h:21-25 — same field order, 48 bytes; `chain` is 0/1 (FWD/REV, common/defs.h:196-197),
   the 'F'/'R' spelling of pairwise_mapping is derived by the caller */
typedef struct {
    int32_t loc1, loc2, left1, left2, right1, right2, score, num1, num2, readno, readstart;
    int32_t chain;
} mhip_candidate;

typedef struct {
    int32_t maxc;            /* -n  MAXC, default 100 (pw_options.cpp:9) */
    int32_t min_align_size;  /* -a  2000 pacbio / 500 nanopore */
    int32_t min_kmer_match;  /* -k  4 / 2 */
    int32_t min_kmer_dist;   /* 1800 / 400 (pw_impl.cpp:845,848) */
    int32_t tech;            /* 0 pacbio (DiffAligner), 1 nanopore */
    double  ddfs_cutoff;     /* 0.25 (pw_impl.cpp:21-23) */
} mhip_params;

/* what mecat2pw consumes of an alignment: go()'s return value, the four coordinates and the identity counts
   (ident = 100.0 * matches / columns is formed by the caller in double, diff_gapalign.h:90-97) */
typedef struct {
    int32_t ok, query_start, query_end, target_start, target_end, matches, columns;
    int32_t blocks;          /* number of 500-bp blocks aligned (work counter) */
} mhip_aln_result;

/* one alignment job: candidate `cand` of query read `qid_local` (index inside the query volume) */
typedef struct {
    int32_t qid_local;       /* read index in the query volume */
    int32_t sid_local;       /* read index in the reference volume (candidate.readno - ref.start_read_id) */
    int32_t chain;           /* 0 forward query, 1 reverse-complemented query */
    int32_t qstart, sstart;  /* extension start points AFTER the +kmer_size/2 adjustment of pw_impl.cpp:681-685 */
} mhip_aln_job;

int  mhip_abi_version(void);
const char* mhip_last_error(void);
int  mhip_device_count(void);

/* Page-locked host memory for the buffers handed to the host-pointer entry points (mhip_seed_reads,
 * mhip_align_candidates ...): optional, any host pointer works, but pageable memory moves at a fraction of the link rate.
 * Additive (the reference has no counterpart: its buffers never leave the host). */
int  mhip_host_alloc(size_t bytes, void** out);
void mhip_host_free(void* p);
/* page-lock / release a caller-owned host buffer around the calls that copy from or into it (0 = locked; a failure leaves it pageable,
 * which only costs copy speed) */
int  mhip_host_register(void* p, size_t bytes);
void mhip_host_unregister(void* p);

/* `stream` may be NULL (the context creates its own) or a hipStream_t the caller owns (e.g. torch's current stream). */
int  mhip_ctx_create(int device, void* stream, mhip_ctx** out);
void mhip_ctx_destroy(mhip_ctx* ctx);
int  mhip_ctx_sync(mhip_ctx* ctx);
/* Optional, additive: allocates the scratch the first mhip_index_build of a volume of up to `bases` bases would allocate
 * (two arrays of 8 bytes per base; tens of GB take hundreds of milliseconds to map).  May run on another thread while the
 * caller still parses its input; every other call on the context that needs scratch waits for it. */
int  mhip_ctx_reserve_index(mhip_ctx* ctx, int64_t bases);
/* for callers that keep tables in HBM between calls (the mecat2pw driver keeps the candidate lists of a whole grid cell there):
   a named device buffer of the context, grown on demand (contents are lost when it grows), freed with the context; and a copy
   from device memory to the host on the context's stream that returns when the bytes have arrived */
int  mhip_ctx_buffer(mhip_ctx* ctx, const char* name, size_t bytes, void** d_ptr);
int  mhip_download(mhip_ctx* ctx, void* host_dst, const void* d_src, size_t bytes);
/* free / total device memory as the driver sees it now (callers size the tables they keep resident from it) */
int  mhip_ctx_mem_info(mhip_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
void mhip_params_default(mhip_params* p, int tech);           /* pw_options.cpp:30-50 + pw_impl.cpp:843-851 */

/* per-kernel timing with HIP events on the context's stream (for bench.py's roofline block).
   set_profiling(1) makes every launch record start/stop events; kernel_stats returns, for the kernel whose name
   matches `name`, the number of launches and the summed duration in ms since the last reset. */
int  mhip_ctx_set_profiling(mhip_ctx* ctx, int on);
int  mhip_ctx_kernel_stats(mhip_ctx* ctx, const char* name, int64_t* launches, double* total_ms);
int  mhip_ctx_kernel_names(mhip_ctx* ctx, char* buf, int buflen);   /* '\n'-separated */
int  mhip_ctx_reset_stats(mhip_ctx* ctx);
/* device work counters accumulated by seed/align calls since the last reset:
   [0] query k-mer lookups  [1] bucket hits H  [2] candidates emitted  [3] dw blocks  [4] d-path cells  [5] snake bases
   [6] aligned query bases  [7] alignments ok */
int  mhip_ctx_counters(mhip_ctx* ctx, int64_t out[8]);

/* volume: host arrays exactly as load_volume() leaves them (pac = (num_bases+3)/4 bytes) */
int  mhip_volume_upload(mhip_ctx* ctx, const uint8_t* pac, const mhip_offset_t* offs, int num_reads, int num_bases,
                        int start_read_id, mhip_volume** out);
/* the same volume made on the device from the residue LETTERS (replaces the packing step of split_raw_dataset,
   common/split_database.cpp:221-266 + PackedDB::set_char, packed_db.h:98-107, unmasked OR of the 4-bit IUPAC value included).
   text = the input file's bytes (host), seq_start[r] = index of read r's first residue, line_width[r] = residues per line of read r (0: one
   line; otherwise every line but the last holds exactly that many and ends in one byte), offs = the volume layout (offset, size; one pad
   base behind every read).  pac_out, when not NULL, receives the (num_bases + 3) / 4 packed bytes (what dump_volume writes). */
int  mhip_volume_pack(mhip_ctx* ctx, const uint8_t* text, int64_t text_bytes, const int64_t* seq_start, const int32_t* line_width,
                      const mhip_offset_t* offs, int num_reads, int num_bases, int start_read_id, mhip_volume** out, uint8_t* pac_out);
void mhip_volume_free(mhip_volume* v);
int  mhip_volume_num_reads(const mhip_volume* v);
int  mhip_volume_num_bases(const mhip_volume* v);

/* index of one volume (k = 13).  Buckets with more than 128 occurrences are empty; bucket contents ascend. */
int  mhip_index_build(mhip_ctx* ctx, const mhip_volume* v, mhip_index** out);
/* the same table with another bucket cap (1..256): mecat2canu's overlappers drop buckets of more than 256 occurrences
   (mecat2asmpw.c:307-314 sumvalue_x) where mecat2pw drops those above 128; everything else about the table is the same */
int  mhip_index_build_ex(mhip_ctx* ctx, const mhip_volume* v, int max_bucket, mhip_index** out);
void mhip_index_free(mhip_index* idx);                       /* waits for the device: work queued through *_dev calls may still read it */
int64_t mhip_index_num_kmers(const mhip_index* idx);
/* parity/debug: counts[4^13] (kept occurrences) and/or offsets[num_kmers]; either may be NULL */
int  mhip_index_download(mhip_ctx* ctx, const mhip_index* idx, int32_t* counts, int32_t* offsets);
/* test hook: the two side arrays the seeding stage reads — slots[num_kmers] ((position / 2000) mod 2^15) and the 16-byte bucket
 * records recs[4^13][4] (start, occurrences below seven position cuts at multiples of *cut_step, occurrences); returns 1 when the
 * table has no records (bucket cap above 255, or not built yet) */
int  mhip_index_download_aux(mhip_ctx* ctx, const mhip_index* idx, uint16_t* slots, uint32_t* recs, int* cut_step);

/* candidates of reads [rid_begin, rid_end) of `reads` against (`ref`, `idx`): for read r the list is written to
   out[(r - rid_begin) * maxc ...] in the reference's list order (score descending, stable), out_counts[r - rid_begin]
   entries.  `out`/`out_counts` are HOST pointers here and DEVICE pointers in the _dev variant (results stay in HBM,
   e.g. for the multi-GPU all-gather). */
int  mhip_seed_reads(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads,
                     int rid_begin, int rid_end, const mhip_params* p, mhip_candidate* out, int32_t* out_counts);
int  mhip_seed_reads_dev(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads,
                         int rid_begin, int rid_end, const mhip_params* p, void* d_out, void* d_out_counts);

/* same for the reads rid_begin + i * rid_stride, i in [0, n): the static multi-GPU shard of a (ref volume, query volume)
   grid cell — rank r of P seeds reads r, r + P, r + 2P, ... (work per read grows with the read id inside a diagonal cell
   because candidates with sid > qid are dropped, pw_impl.cpp:370, so the shard is cyclic, not contiguous) */
int  mhip_seed_reads_strided_dev(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads,
                                 int rid_begin, int rid_stride, int n, const mhip_params* p, void* d_out, void* d_out_counts);

/* candidate lists -> alignment jobs, on the device (the loop head of pairwise_mapping, pw_impl.cpp:674-686: the
   +kmer_size/2 shift of both start points only when both are non-zero).  d_cands[n_reads][maxc], d_counts[n_reads];
   read i of the table is query read rid_begin + i * rid_stride.  Only jobs with (job index % part_count) == part_index
   are emitted (multi-GPU split of the extension stage; 0/1 = all).  d_jobs must hold n_reads * maxc entries;
   *num_jobs receives the number written. */
int  mhip_jobs_from_candidates_dev(mhip_ctx* ctx, const void* d_cands, const void* d_counts, int n_reads, int maxc,
                                   int rid_begin, int rid_stride, int ref_start_read_id, int part_index, int part_count,
                                   void* d_jobs, int* num_jobs);

/* the occupied entries of a candidate table, dense and read-major: d_pack[first(i) + k] = d_cands[i][k] with first = exclusive prefix
   sum of d_counts; *total = number of entries.  d_pack must hold them (n_reads * maxc entries always suffice). */
int  mhip_pack_candidates_dev(mhip_ctx* ctx, const void* d_cands, const void* d_counts, int n_reads, int maxc, void* d_pack, int64_t* total);

/* dw extension of n jobs (PacBio / DiffAligner semantics); jobs/out are HOST pointers (_dev: DEVICE pointers) */
int  mhip_align_candidates(mhip_ctx* ctx, const mhip_volume* ref, const mhip_volume* reads, const mhip_aln_job* jobs,
                           int n, int min_align_size, mhip_aln_result* out);
int  mhip_align_candidates_dev(mhip_ctx* ctx, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs,
                               int n, int min_align_size, void* d_out);

/* the same contract with XdropAligner semantics (nanopore mode, common/xdrop_gapalign.cpp:359-439: reward 1, penalty -1,
   gap_open 0, gap_extend 1, X = 30; ok = query_end - query_start >= min_align_size; `columns`/`matches` count the
   reference's aligned strings, whose left half is emitted without its last column) */
int  mhip_xalign_candidates(mhip_ctx* ctx, const mhip_volume* ref, const mhip_volume* reads, const mhip_aln_job* jobs,
                            int n, int min_align_size, mhip_aln_result* out);
int  mhip_xalign_candidates_dev(mhip_ctx* ctx, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs,
                                int n, int min_align_size, void* d_out);

/* ---- multi-GPU: one process per GPU, the all-vs-all grid sharded statically, candidate lists exchanged over
 * RCCL.  The reference parallelises a grid cell (reference volume i x query volume j) over pthreads pulling chunks of 500 query
 * reads from a shared cursor (mecat2pw/pw_impl.cpp:612-621, 866-876); here chunk c of query volume j belongs to rank
 * (c + cell_shift) mod nranks (the driver passes cell_shift = j).  Every rank builds the index of volume i itself
 * (mhip_index_build: recompute beats moving it), seeds the reads of its own chunks, and ONE count-then-payload all-gather per
 * slab of reads leaves the complete candidate table on every rank: one int32 per read first, then only the occupied 48-byte
 * records, sent directly to every peer (xGMI is point to point).  Nothing here has a counterpart in the reference.
 *
 * mhip_comm_unique_id / mhip_comm_init wrap ncclGetUniqueId / ncclCommInitRank (RCCL is opened lazily, single-GPU runs never
 * load it): rank 0 creates the id and hands it to the other ranks by any means (the driver uses a file in wrk_dir, bench.py a
 * torch.distributed broadcast).  Collectives run on the context's stream.  mhip_comm_init_hostfile is a TEST HOOK for boxes
 * with fewer GPUs than ranks (RCCL refuses two ranks on one device): same calls, transport through files in `dir`. */
typedef struct mhip_comm mhip_comm;
#define MHIP_COMM_ID_BYTES 128
#define MHIP_SHARD_CHUNK 500       /* CHUNK_SIZE, mecat2pw/pw_impl.h:15 */
int  mhip_comm_unique_id(uint8_t id[MHIP_COMM_ID_BYTES]);
int  mhip_comm_init(mhip_ctx* ctx, int nranks, int rank, const uint8_t id[MHIP_COMM_ID_BYTES], mhip_comm** out);
int  mhip_comm_init_hostfile(mhip_ctx* ctx, int nranks, int rank, const char* dir, const char* run_id, mhip_comm** out);
void mhip_comm_destroy(mhip_comm* comm);
/* transport: 0 = RCCL, 1 = host files (test hook); rccl_ranks = ncclCommCount of the communicator (0 with host files).  With the
 * context profiling (mhip_ctx_set_profiling) every exchange is timed on the stream under the kernel-stat names "xg_exchange"
 * (candidate / result all-gathers) and "xg_exchange_index" (mhip_index_build_sharded). */
int  mhip_comm_info(const mhip_comm* comm, int* transport, int* rccl_ranks);      /* transport 0 RCCL, 1 host files, 2 none (solo) */
/* BENCH HOOK (bench.py --simulate-ranks): rank `rank` of `nranks` with no transport.  The sharded calls below then do exactly this rank's
 * share of the work on the device — its key range of mhip_index_build_sharded, its chunks in mhip_seed_reads_sharded / mhip_align_sharded,
 * the pack and scatter kernels of the exchanges — and its peers' contributions read as zero counts: what one rank of P computes, timed
 * alone.  mhip_comm_bytes_sent = the bytes this rank's contributions put on the links (its bytes x (P - 1) peers), in any transport. */
int  mhip_comm_init_solo(mhip_ctx* ctx, int nranks, int rank, mhip_comm** out);
int64_t mhip_comm_bytes_sent(const mhip_comm* comm);
int64_t mhip_comm_local_jobs(const mhip_comm* comm);         /* candidates of this rank's own reads in the last mhip_seed_reads_sharded slab */
int  mhip_comm_rank(const mhip_comm* comm);
int  mhip_comm_nranks(const mhip_comm* comm);
int  mhip_comm_barrier(mhip_comm* comm);
int  mhip_comm_selftest(mhip_ctx* ctx);                       /* RCCL loads and moves bytes on this device (one-rank communicator) */
int64_t mhip_comm_bytes_received(const mhip_comm* comm);      /* payload + counts received from peers so far */

/* shard arithmetic for the reads [rid_begin, rid_end) of a query volume (rid_begin must be a multiple of chunk): how many of
 * them `rank` owns and the first one; local index i is read first + (i / chunk) * chunk * nranks + i % chunk */
int  mhip_shard_local_count(int rid_begin, int rid_end, int chunk, int cell_shift, int rank, int nranks);
int  mhip_shard_first_read(int rid_begin, int rid_end, int chunk, int cell_shift, int rank, int nranks);
/* rows mode (#volumes >= ranks: a grid row per GPU, no data moves): the static deal of the rows still to do.  Row i of the upper
 * triangular volume grid holds the cells (i, i) .. (i, num_vols - 1) (mecat2pw/pw.cpp:65-81, pw_impl.cpp:859-879), so a row costs
 * num_vols - i cell visits (+ one index build, priced at a quarter of a cell); rows are taken heaviest first and each goes to the rank
 * with the least work so far (ties: the lowest rank) — 19 rows over 8 ranks: heaviest rank 26 cells against a mean of 23.75, where the
 * cyclic deal i mod P gave 33.  Every rank derives the same deal from the split marker alone.  owner[i] = the rank of row i, -1 for a
 * row that is not in todo[].  Returns the heaviest rank's cell count, -1 on bad arguments. */
int  mhip_shard_deal_rows(int num_vols, const int* todo, int ntodo, int nranks, int* owner /*[num_vols]*/);
/* mhip_seed_reads_dev for the local reads of such a shard (first = mhip_shard_first_read, n = mhip_shard_local_count) */
int  mhip_seed_reads_chunked_dev(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int first,
                                 int chunk, int nranks, int n, const mhip_params* p, void* d_out, void* d_out_counts);

/* The exchange step: d_cands[n_local][maxc] / d_counts[n_local] are this rank's lists (DEVICE pointers); on return
 * d_all_cands[rid_end - rid_begin][maxc] / d_all_counts[rid_end - rid_begin] hold the complete table of the slab, read-major,
 * on every rank — the layout mhip_seed_reads produces. */
int  mhip_allgather_candidates(mhip_comm* comm, const void* d_cands, const void* d_counts, int rid_begin, int rid_end, int chunk,
                               int cell_shift, int maxc, void* d_all_cands, void* d_all_counts);

/* mhip_seed_reads over all ranks: seeds this rank's chunks of [rid_begin, rid_end) and exchanges.  out / out_counts are HOST
 * pointers in mhip_seed_reads' layout and may be NULL (the table stays on the device, see mhip_sharded_tables). */
int  mhip_seed_reads_sharded(mhip_comm* comm, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin,
                             int rid_end, int chunk, int cell_shift, const mhip_params* p, mhip_candidate* out, int32_t* out_counts);
/* mhip_align_candidates / mhip_xalign_candidates (tech 0 / 1) over all ranks, for the slab of the preceding
 * mhip_seed_reads_sharded call: every rank extends the candidates of its own reads, the 32-byte results are exchanged like the
 * candidates.  out (HOST, may be NULL) receives one result per candidate, read-major: read rid_begin's candidates in list order,
 * then read rid_begin + 1's ... — the order of the job list the driver builds from the table.  *num_jobs = their number. */
int  mhip_align_sharded(mhip_comm* comm, const mhip_volume* ref, const mhip_volume* reads, int tech, int min_align_size,
                        mhip_aln_result* out, int64_t* num_jobs);
/* device views of the tables the last two calls left on this rank (complete on every rank) */
int  mhip_sharded_tables(mhip_comm* comm, void** d_cands, void** d_counts, void** d_results, int64_t* num_jobs);
/* ---- mecat2canu's overlapper for corrected reads (mecat2asmpw / mecat2trimpw), candidate stage ----
 * Replaces the part of pairwise_mapping in front of its extension loop (mecat2canu/src/mecat2asmpw/mecat2asmpw.c:580-718): seeding of
 * both strands of query reads [rid_begin, rid_end) of `reads` against one block of reads (`block`: the tool's STRMEM as a volume — one
 * pad base after every read is the tool's one NUL after every read, so offsets agree; start_read_id = the block's first read number)
 * whose table was built with mhip_index_build_ex(ctx, block, 256, ..) (creat_ref_index + sumvalue_x: cap 256), and candidate
 * selection.  out[(rid - rid_begin) * 100 .. ] = the read's candidates in list order (canidate_save, :55-58; positions 1-based as in
 * the tool, chain 0 = 'F', 1 = 'R'), out_counts[] their number (<= 100).  Every read starts from an all-zero segment array (the
 * tool's worker threads keep stale seeds of the reads they mapped before, which can move a score by a few votes: INTEGRATION.md). */
typedef struct { int32_t loc1, loc2, left1, left2, right1, right2, score, num1, num2, readno, readstart, chain; } mhip_asm_candidate;
/* Bases other than A, C, G, T (an N of a corrected read): the tools restart their k-mer at such a base in table and query
 * (mecat2asmpw.c:445, 486, 316-335) and compare it as a character in the extension (N equals N only).  A volume may carry a second
 * plane in its own 2-bit layout — 3 at every such base (stored as code 0 in the volume), 0 elsewhere; nplane = (num_bases + 3) / 4 bytes,
 * NULL removes it.  mhip_asm_seed_reads skips the query k-mers that touch one, mhip_asm_extend compares with both planes; the table of a
 * block with such bases is built from a volume whose read table ends a "read" at every one of them (the index never starts a k-mer inside
 * the 13 positions in front of a read end: exactly the positions whose 13-mer would hold the base). */
int  mhip_volume_set_nplane(mhip_ctx* ctx, mhip_volume* vol, const uint8_t* nplane);
int  mhip_asm_seed_reads(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* block, const mhip_volume* reads, int rid_begin,
                         int rid_end, mhip_asm_candidate* out, int32_t* out_counts);
int  mhip_asm_seed_reads_ex(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* block, const mhip_volume* reads, int rid_begin,
                            int rid_end, int gate /*10: mecat2asmpw, 8: mecat2trimpw*/, int maxc /*100; 50: the *50 variants*/,
                            mhip_asm_candidate* out /*[n][100]*/, int32_t* out_counts);
/* The tool's extension loop (mecat2asmpw.c:723-841: blocks of 500 bases while more than 600 remain, O(ND) `align` at error rate 0.10,
 * a block's tail cut in front of its last run of four matches) for a batch of (candidate, both directions) jobs.  A job names the two
 * reads (xid in `block`, yid in `reads`), the strand of the mapped read, and per direction the start positions (local to the read /
 * to the mapped strand) and the bases available: from a candidate c of query read r, with x0 = c.loc1 - 1 - c.readstart,
 *   left   lx = x0 + 12, ly = c.loc2 + 12, lnx = c.left1, lny = c.left2      (backwards from the LAST base of the seed 13-mer)
 *   right  rx = x0,      ry = c.loc2,      rnx = c.right1, rny = c.right2    (forwards from its first base)
 * dirs[2 i + d] = {columns, x bases, y bases, y-only columns, x-only columns, 0} of direction d (0 left, 1 right);
 * ops[(2 i + d) * dir_cols_cap / 16 ...] the columns, 2 bits each, in extension order: 0 = both bases (always equal: O(ND) paths have
 * no mismatch columns), 1 = y base only, 2 = x base only.  The bits behind a direction's last column are zero. */
typedef struct { int32_t xid, yid, chain, lx, ly, lnx, lny, rx, ry, rnx, rny, pad; } mhip_asm_job;
int  mhip_asm_extend(mhip_ctx* ctx, const mhip_volume* block, const mhip_volume* reads, const mhip_asm_job* jobs, int n, int dir_cols_cap,
                     int32_t* dirs /*[2 n][6]*/, uint32_t* ops /*[2 n][dir_cols_cap / 16]*/);
/* The same extension with the columns handed over densely, in two calls (what the tools use: a direction fills a fraction of
 * dir_cols_cap, so the fixed-stride form moves 5-10x the bytes over the PCIe link).  mhip_asm_extend_run extends the batch, leaves the
 * results on the device and returns the number of 32-bit words the columns of all directions take (ceil(columns / 16) per direction);
 * mhip_asm_extend_fetch — same context, same n, before the next _run — copies them out: direction k = 2 i + d occupies words
 * [word_offs[k], word_offs[k + 1]) of ops_dense (total_words words).  Host buffers from mhip_host_alloc make the copies DMA. */
int  mhip_asm_extend_run(mhip_ctx* ctx, const mhip_volume* block, const mhip_volume* reads, const mhip_asm_job* jobs, int n, int dir_cols_cap,
                         int64_t* total_words);
int  mhip_asm_extend_fetch(mhip_ctx* ctx, int n, int32_t* dirs /*[2 n][6]*/, uint64_t* word_offs /*[2 n + 1]*/, uint32_t* ops_dense /*[total_words]*/);

/* ---- mecat2ref, the reads-to-reference mapper, stage 1: seeding and candidate selection ----
 * Replaces the part of reference_mapping in front of its extend_candidate loop (mecat2ref/mecat2ref_impl_large.cpp:351-561 for the first
 * round, :619-825 for the second, with transnum_buchang :64-90, insert_loc :92-130 and find_location, mecat2ref_aux.cpp:6-83): both
 * strands of query reads [rid_begin, rid_end) of `reads` against the reference volume `ref` (mecat_amd/host/ref_genome.h makes it from
 * the FASTA file) whose table is mhip_index_build's (creat_ref_index :133-271 with sumvalue_x :53-62: k = 13, cap 128).  A query k-mer
 * that holds a letter other than upper-case A, C, G, T is skipped (atcttrans :44-51; the tool does not upper-case reads): `reads` carries
 * an N plane (mhip_volume_set_nplane) that is 3 at every such letter.  Every read starts from untouched segments (:605-616).
 * out[(rid - rid_begin) * maxc ..] = the read's candidates in list order (forward strand first, stable by descending score, at most
 * maxc), out_counts[] their number.  Positions are the tool's: loc1 the 1-based start of the seed 13-mer in the concatenated reference,
 * loc2 the 0-based start in the mapped strand of the read.  Refused with a message: a read of 100 000 letters or more (RM, the tool's
 * buffers).  A read shorter than 13 letters has no candidates (the tool reads past the string there). */
typedef struct { int64_t loc1, loc2, left1, left2, right1, right2; int32_t score, num1, num2, chain; } mhip_ref_candidate; /* candidate_save, mecat2ref_defs.h:88-93; chain 0 = 'F', 1 = 'R' */
typedef struct { int32_t maxc; int32_t round; double ddfs_cutoff; } mhip_ref_seed_params;  /* round 0: ZV 1000, BC by length, gate 6; 1: ZVS 2000, BC 5, gate 4 */
/* maxc 10 (kDefaultNumCandidates, mecat2ref.cpp:18), round 0, cutoff 0.25 for BOTH technologies: mecat2ref_impl_large.cpp:13-15 names
 * 0.1 for nanopore and never assigns it, so the tool maps nanopore reads at 0.25 too (a caller may still set 0.1) */
void mhip_ref_seed_params_default(mhip_ref_seed_params* p, int tech);
int  mhip_ref_seed_reads(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                         const mhip_ref_seed_params* params, mhip_ref_candidate* out /*[n][maxc]*/, int32_t* out_counts);
/* the same with DEVICE pointers for out / out_counts (the lists stay in HBM for the extension stage) */
int  mhip_ref_seed_reads_dev(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                             const mhip_ref_seed_params* params, mhip_ref_candidate* d_out, int32_t* d_out_counts);
/* measurement hook: of the last mhip_ref_seed_reads* call — [0] reads, [1] reads redone with full record pools, [2] resident waves,
 * [3] records per pool */
void mhip_ref_seed_stats(int64_t out[4]);

/* ---- mecat2ref, stage 2: every listed candidate through DiffAligner::go, with the aligned strings (PacBio mode) ----
 * Replaces the extend_candidate loop of reference_mapping (mecat2ref/mecat2ref_impl_large.cpp:566-582 for round 1, :829-845 for round 2)
 * with extend_candidate (mecat2ref_aux.cpp:123-183), extract_sequences (:85-121) and DiffAligner::go (common/diff_gapalign.cpp:294-349;
 * blocks, band, best-point fallback, tail anchor and traceback :39-292, common/gapalign.cpp:9-68).  cands / counts are
 * mhip_ref_seed_reads' output for the same reads [rid_begin, rid_end) and maxc; slot (read, k) of the result is slot (read, k) of the list,
 * which is the tool's call order.  The target of a candidate is the window [loc1 - 1 - left_ref_size, loc1 - 1 + right_ref_size) of the
 * concatenated reference (`ref`: mecat_amd/host/ref_genome.h), the query the read on the candidate's strand.  The strand is the tool's:
 * the whole read reversed, only upper-case A, C, G, T complemented (:376-410) — `reads` must be packed by mecat_amd/host/ref_reads.h
 * (lower-case a, c, g, t keep their codes, N plane 3 there and at every other letter; the plane is what keeps a base from being
 * complemented).  A result: ok = columns >= 1000 (the tool keeps only those), chain / vscore of the candidate, qb / qe / qs and sb / se as
 * extend_candidate stores them (:158-162), cols = the length of the aligned strings.  The strings are 2-bit columns in string order,
 * 16 per word from the low end: 0 = both bases, 1 = target base only ('-' in the query string), 2 = query base only
 * (mecat_amd/host/ref_results.h rebuilds the text).  Empty slots and results with ok = 0 take zero words.
 * mhip_ref_extend_run extends the batch, leaves everything on the device and returns the words the ok results take;
 * mhip_ref_extend_fetch — same context, before the next _run — copies out res[n * maxc], word_offs[n * maxc + 1] (result s occupies words
 * [word_offs[s], word_offs[s + 1]) of ops_dense) and the words.  Refused with a message (-1): tech != 0 (nanopore mode has calls of its
 * own, mhip_ref_xextend_run below), a read of 100 000 letters or more (RM), a candidate whose loc1 or loc2 lies outside the reference or
 * the read (nothing is extended then). */
typedef struct { int32_t ok, chain, vscore, qb, qe, qs; int64_t sb, se; int32_t cols, pad; } mhip_ref_result;   /* TempResult without its strings, mecat2ref_defs.h */
int  mhip_ref_extend_run(mhip_ctx* ctx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc, int tech,
                         const mhip_ref_candidate* cands /*[n][maxc]*/, const int32_t* counts, int64_t* total_words);
/* the same with DEVICE lists: mhip_ref_seed_reads_dev's output, nothing copied back in between */
int  mhip_ref_extend_run_dev(mhip_ctx* ctx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc, int tech,
                             const mhip_ref_candidate* d_cands, const int32_t* d_counts, int64_t* total_words);
int  mhip_ref_extend_fetch(mhip_ctx* ctx, mhip_ref_result* res /*[n][maxc]*/, uint64_t* word_offs /*[n * maxc + 1]*/, uint32_t* ops_dense /*[total_words]*/);
/* measurement hook: of the last mhip_ref_extend_run* call — [0] slots, [1] slices, [2] bytes of row scratch, [3] words of the column store */
void mhip_ref_extend_stats(int64_t out[4]);

/* ---- mecat2ref, stage 2 in nanopore mode (`-x 1`): the same candidates through XdropAligner::go, with the aligned strings ----
 * The technology changes one thing in the tool: reference_mapping creates an XdropAligner instead of a DiffAligner
 * (mecat2ref_impl_large.cpp:328-335).  Same arguments as mhip_ref_extend_run* without `tech`, the same jobs, windows, strand rule, slices
 * and refusals; the results go to the same buffers, so mhip_ref_extend_fetch fetches them.  What differs (common/xdrop_gapalign.cpp:
 * 263-439): the blocks are affine X-drop extensions (reward 1, penalty -1, gap 0 / 1, X = 30), the left half is joined without its last
 * column (:401-402), and ok = qe - qb >= 1000 — the QUERY SPAN (:438), not the columns: a result with 1000 columns and a shorter span
 * is not ok, cols = aln_size either way.  X-drop paths hold substitutions over unequal bases: a column of code 0 takes a base of each
 * sequence and the two may differ (mismatch columns); mecat_amd/host/ref_results.h writes the letters, which tell them apart.
 * MECAT_XD_WIDE=1 (read at call time) sends every block through the wide block: the ring block's cross-check. */
int  mhip_ref_xextend_run(mhip_ctx* ctx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc,
                          const mhip_ref_candidate* cands /*[n][maxc]*/, const int32_t* counts, int64_t* total_words);
int  mhip_ref_xextend_run_dev(mhip_ctx* ctx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end, int maxc,
                              const mhip_ref_candidate* d_cands, const int32_t* d_counts, int64_t* total_words);
/* measurement hook: of the last mhip_ref_xextend_run* call — [0] slots, [1] slices, [2] blocks redone with the wide block (their window
 * outgrew the ring block's 128 cells: low-complexity sequence), [3] words of the column store */
void mhip_ref_xextend_stats(int64_t out[4]);

/* ---- mecat2ref, stage 3: the clipped-alignment rescue and the result order (PacBio mode) ----
 * Replaces everything of reference_mapping between its extension loop and the per-thread result file (mecat2ref_impl_large.cpp:584-603
 * for round 1, :847-866 for round 2): rescue_clipped_align (mecat2ref/mecat2ref_aux.cpp:308-452) with find_left_clipped_candidate /
 * find_right_clipped_candidate / fill_clipped_candidate (:185-274), is_left_clipped_align / is_right_clipped_align (:276-306),
 * is_full_align and AlignInfoContained (mecat2ref_aux.h:22-42), and output_results (:454-473).  Input: the results of the read's first
 * list (mhip_ref_extend_run's, maxc <= 10).  The searches need the per-segment seed records (Back_List) of the strands that own one of a
 * read's first three entries; stage 1 does not keep them, so its seeding loop (mecat2ref_impl_large.cpp:417-453) runs again for the reads
 * the tool does not return early on.  The rescue candidates (at most 6 per read, in the tool's call order) go through the same
 * extension as the lists, into a second set of buffers: mhip_ref_extend_fetch still returns the first extension afterwards.
 * A record is named by its slot: [0, maxc) is a slot of the read's first list (mhip_ref_extend_fetch's res[n][maxc]), maxc + j is rescue
 * slot j of the read.  out_slots[n][3 * num_output] holds, per read, the slots in the order output_results prints their records
 * (out_counts[n] of them, the rest -1): mecat_amd/host/ref_results.h writes the records.
 * mhip_ref_rescue_state, what :328-341 leave: naln surviving entries in the sorted order, entry k = list slot slot[k] with the tool's id
 * id[k] (its index among the read's ok results); nres = ok results of the first list (the id the first ok rescue result takes); qs = the
 * read's length; go_on = 0 when the tool returns at :341 (the longest entry covers 0.9 of the read) or there is no entry.
 * Refused with a message and -1, the context stays usable: tech != 0 (nanopore mode: mhip_ref_xrescue_run), maxc outside 1..10 (std::sort's order of equal lengths is
 * reproduced for at most 16 entries), num_output < 1, round outside 0..1, a read of 100 000 letters or more, an index that was not
 * built from this reference. */
typedef struct { int32_t maxc, round, num_output, tech; double ddfs_cutoff; } mhip_ref_rescue_params;
typedef struct { int32_t naln, go_on, nres, qs; int8_t slot[16], id[16]; } mhip_ref_rescue_state;
/* maxc 10 (kDefaultNumCandidates, mecat2ref.cpp:18), round 0, num_output 10 (kDefaultNumOutput, :19), tech, ddfs_cutoff 0.25 */
void mhip_ref_rescue_params_default(mhip_ref_rescue_params* p, int tech);
/* res: HOST results [n][maxc] of reads [rid_begin, rid_end) (mhip_ref_extend_fetch's layout); total_words = the words the ok rescue results take */
int  mhip_ref_rescue_run(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                         const mhip_ref_rescue_params* params, const mhip_ref_result* res /*[n][maxc]*/, int64_t* total_words);
/* the same on DEVICE results; d_res = NULL: the results of the last mhip_ref_extend_run* on this context (refused if that run's slots
 * are not n * maxc) */
int  mhip_ref_rescue_run_dev(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                             const mhip_ref_rescue_params* params, const mhip_ref_result* d_res, int64_t* total_words);
/* Nanopore mode: stage 3 with the X-drop extension (mhip_ref_xextend_run's) behind the rescue candidates.  Prep, the searches, the
 * re-seeding, the attach tests and the output order do not depend on the technology; the extension and its ok rule do.  params->tech
 * must be 1 (as mhip_ref_rescue_run wants 0: a caller that mixes the two up is told); the other refusals are the PacBio calls'.
 * Results are fetched by mhip_ref_rescue_fetch. */
int  mhip_ref_xrescue_run(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                          const mhip_ref_rescue_params* params, const mhip_ref_result* res /*[n][maxc]*/, int64_t* total_words);
int  mhip_ref_xrescue_run_dev(mhip_ctx* ctx, const mhip_index* idx, const mhip_volume* ref, const mhip_volume* reads, int rid_begin, int rid_end,
                              const mhip_ref_rescue_params* params, const mhip_ref_result* d_res, int64_t* total_words);
/* same context, before the next mhip_ref_rescue_run*: rescue_cands / rescue_res [n][6] (entries behind rescue_counts[i] are undefined),
 * word_offs[6 n + 1] and ops_dense[total_words] as mhip_ref_extend_fetch gives them for the rescue results */
int  mhip_ref_rescue_fetch(mhip_ctx* ctx, int32_t* out_slots /*[n][3 * num_output]*/, int32_t* out_counts, mhip_ref_candidate* rescue_cands,
                           int32_t* rescue_counts, mhip_ref_result* rescue_res, uint64_t* word_offs, uint32_t* ops_dense);
/* measurement hook: of the last mhip_ref_rescue_run* call — [0] reads, [1] reads that went on past :341, [2] rescue candidates,
 * [3] reads redone with full record pools */
void mhip_ref_rescue_stats(int64_t out[4]);
/* test hook: ref_rescue_prep (:328-341) on host results res[n][maxc] -> states[n] */
int  mhip_debug_ref_rescue_prep(mhip_ctx* ctx, const mhip_ref_rescue_params* params, int n, const mhip_ref_result* res /*[n][maxc]*/,
                                mhip_ref_rescue_state* states /*[n]*/);
/* test hook: ref_rescue_finish — the attach tests of :380-399 / :416-435 on the rescue results in call order, :438-451 and
 * output_results — on hand-made states and rescue results.  rescue_meta[n][6]: owner entry (place in the state's order, 0..2) |
 * side << 8 (0 left, 1 right); rescue_res[n][6]; out_slots[n][3 * num_output] (unused places -1), out_counts[n] = records printed. */
int  mhip_debug_ref_rescue_finish(mhip_ctx* ctx, const mhip_ref_rescue_params* params, int n, const mhip_ref_result* res /*[n][maxc]*/,
                                  const mhip_ref_rescue_state* states, const int32_t* rescue_counts, const int32_t* rescue_meta,
                                  const mhip_ref_result* rescue_res, int32_t* out_slots, int32_t* out_counts);

/* mhip_index_build by all ranks of the communicator together (replaces create_ref_index, common/lookup_table.cpp:63-160, in a
 * multi-GPU cell): the 4^13 key space is cut into P contiguous ranges of equal occupancy, each rank builds the buckets of its range,
 * positions and table slices are all-gathered (counts first, then payload), and every rank returns the complete table — equal, array
 * for array, to the one mhip_index_build makes.  Collective: every rank of `comm` calls it with the same volume. */
int  mhip_index_build_sharded(mhip_comm* comm, const mhip_volume* v, mhip_index** out);
/* The faster of mhip_index_build on every rank and mhip_index_build_sharded, decided by measurement: the first call on a communicator runs
 * both (once to warm up, once timed barrier to barrier; the slowest rank's time counts) and keeps the faster one for this and every later
 * call; MECAT_HIP_INDEX_SHARD=0 / 1 decides without measuring.  ms[0] / ms[1] (may be NULL): the replicated / sharded build times the
 * decision rests on, 0 when nothing was measured; *sharded (may be NULL): what was used.  No counterpart in the reference. */
int  mhip_index_build_auto(mhip_comm* comm, const mhip_volume* v, mhip_index** out, double ms[2], int* sharded);

/* ---- mecat2cns re-aligner: ns_banded_sw::GetAlignment of src/mecat2cns/dw.cpp:482-553, which
 * mecat2cns calls for up to 200 candidates per template read (mecat_correction.cpp:286, 347, 431, 494) -------------------
 * Jobs are mhip_aln_job records: qid_local = the candidate read in `reads`, taken reverse-complemented when chain != 0;
 * sid_local = the template read in `ref`; qstart / sstart = the extension start (qext, sext).  error_rate is 0.15 (PacBio)
 * or 0.20 (nanopore), <= 0.20.  An O(ND) alignment has no mismatch columns, so a column is 0 = both bases (equal),
 * 1 = target base only (gap in the query string), 2 = query base only (gap in the target string): 2 bits per column,
 * 16 columns per uint32 from the least significant bits, dir_cols_cap columns (a multiple of 16) per direction:
 *   ops[(2 * i    ) * dir_cols_cap / 16 ...]  left  direction of job i, in extension order (outwards from the start point)
 *   ops[(2 * i + 1) * dir_cols_cap / 16 ...]  right direction
 * The reference's merged strings are reverse(left) + right; GetAlignment keeps merged columns [first_col, last_col). */
typedef struct mhip_cns_result {
    int32_t ok;                                  /* GetAlignment's return value */
    int32_t qoff, qend, soff, send;              /* m5qoff / m5qend / m5soff / m5send */
    int32_t left_cols, right_cols;               /* columns stored per direction */
    int32_t first_col, last_col;                 /* the aligned strings are merged columns [first_col, last_col) */
    int32_t mat, ins, del;                       /* OutputStore counts over the untrimmed string (dw.cpp:441-470) */
    int32_t query_start, query_end, target_start, target_end;    /* OutputStore coordinates before GetAlignment's trimming */
} mhip_cns_result;

int mhip_cns_align_candidates(mhip_ctx* ctx, const mhip_volume* ref, const mhip_volume* reads, const mhip_aln_job* jobs, int n,
                              double error_rate, int min_align_size, int dir_cols_cap, mhip_cns_result* results, uint32_t* ops);
int mhip_cns_align_candidates_dev(mhip_ctx* ctx, const mhip_volume* ref, const mhip_volume* reads, const void* d_jobs, int n,
                                  double error_rate, int min_align_size, int dir_cols_cap, void* d_results, void* d_ops);

/* ---- mecat2cns' candidate accept loop (BASELINE config 4): the front half of
 * consensus_one_read_can_pacbio / _nanopore (mecat2cns/mecat_correction.cpp:388-450, 452-515) for a batch of template reads.
 * cands: ExtensionCandidate records (common/alignment.h:8-19, the 13 ints of a .can line as mecat2cns normalises them: sdir == 0,
 * sid = the template), grouped by template: template t owns cands[tmpl_begin[t] .. tmpl_begin[t + 1]); they are sorted IN PLACE by
 * (score desc, qid, qext) as the reference does.  All reads live in `vol` (host_pac, the packed bytes given to mhip_volume_upload, is no
 * longer read and may be NULL: since round 6 the aligned strings are built on the device and copied into the result buffer).
 * tech 0: error rate 0.15, at most 60 accepted; tech 1: 0.20 / 100.  min_mapping_ratio is the option value (0.9 / 0.4), the
 * function subtracts the reference's 0.02.  Output (malloc'ed, release with mhip_cns_free): one record per accepted alignment
 * in the order the reference would add them, template by template, and the gap-normalised aligned strings
 * (normalize_gaps(.., push = true), reads_correction_aux.cpp:3-81) that meap_add_one_aln / CnsAlns::add_aln consume:
 * strings + str_offset = qaln (aln_size chars + NUL), then saln (aln_size chars + NUL).
 * Ties: candidates equal in (score, qid, qext) keep the order the reference's own std::sort gives them when cands[] arrives in the
 * reference's order (the partition file's); any other input order may accept tied records in another order.  Every record's
 * qsize / ssize must equal the volume's read lengths (refused otherwise). */
typedef struct { int32_t qdir, qid, qext, qsize, qoff, qend, sdir, sid, sext, ssize, soff, send, score; } mhip_ext_candidate;
typedef struct {
    int32_t template_index;      /* index into tmpl_begin */
    int32_t qid, sid;
    int32_t qoff, qend, soff, send;          /* m5qoff / m5qend / m5soff / m5send */
    int32_t aln_size;
    int64_t cand_index;          /* position of the candidate in cands[] (after the in-place sort) */
    int64_t str_offset;
} mhip_cns_accepted;
int  mhip_cns_accept_templates(mhip_ctx* ctx, const mhip_volume* vol, const uint8_t* host_pac, mhip_ext_candidate* cands,
                               const int64_t* tmpl_begin, int num_templates, int tech, int min_align_size, double min_mapping_ratio,
                               int num_threads, mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings,
                               int64_t* out_strings_bytes, int64_t* out_jobs /* alignments computed, may be NULL */);
void mhip_cns_free(void* p);
/* test hook: normalize_gaps' gap pushing (reads_correction_aux.cpp:36-67) by the device kernel of the accept stage, in place, on n_pairs
 * pairs of NUL-terminated host strings: pair p = buf + off[p] (len[p] characters + NUL) and its partner right behind it */
int  mhip_debug_push_gaps(mhip_ctx* ctx, char* buf, int64_t bytes, const int64_t* off, const int32_t* len, int n_pairs);
/* ---- mecat2cns' consensus table, built in the accept stage (cns_table.hip).  The first thing the reference does with the strings of
 * an accepted alignment is to fold them into the template's table of CnsTableItem {base, mat_cnt, ins_cnt, del_cnt}
 * (reads_correction_aux.h:11-19): meap_add_one_aln, mecat_correction.cpp:36-60, called at :439 / :502; it then classifies every
 * position (identify_one_consensus_item, :14-24: FMAT 1, FDEL 2, FINS 4, UNDS 8) and only positions flagged UNDS or FDEL look at the
 * strings again (meap_consensus_one_segment, :81-108).  mhip_cns_accept_templates_ex is mhip_cns_accept_templates (same arguments
 * without host_pac, same accepted records and strings) with `want` choosing the outputs:
 *   MHIP_CNS_WANT_STRINGS   the aligned strings, as before
 *   MHIP_CNS_WANT_TABLE     the tables and ident bytes of all templates: template t owns out_table[out_table_begin[t] ..
 *                           out_table_begin[t + 1]), one item per base of the template read (whole read: positions no alignment
 *                           covers hold {'N', 0, 0, 0} and ident 7, as in the reference's cleared table), no items for a template
 *                           without candidates; out_ident is indexed alike; out_table_begin has num_templates + 1 entries.  `base` is
 *                           the template's own letter where mat_cnt > 0 — what every match column writes there — else 'N'.
 * With MHIP_CNS_WANT_TABLE alone the strings are built on the device (the tally reads them) but never copied: *out_strings is NULL,
 * *out_strings_bytes 0 and str_offset -1 in every accepted record.  want == 0 is an error.  Outputs that were not asked for come back
 * NULL (their pointers may be NULL then); all are released with mhip_cns_free.  Counts are bytes: at most 60 / 100 alignments are
 * accepted per template, so none overflows.  Effective ranges and segment cutting: mhip_cns_accept_templates_plan below; the POA
 * refinement stays with the caller. */
typedef struct { uint8_t base, mat_cnt, ins_cnt, del_cnt; } mhip_cns_table_item;   /* CnsTableItem */
#define MHIP_CNS_WANT_STRINGS 1
#define MHIP_CNS_WANT_TABLE   2     /* table + ident */
int  mhip_cns_accept_templates_ex(mhip_ctx* ctx, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin,
                                  int num_templates, int tech, int min_align_size, double min_mapping_ratio, int num_threads, int want,
                                  mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings, int64_t* out_strings_bytes,
                                  int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident,
                                  int64_t** out_table_begin /* [num_templates + 1] */);
/* test hook: the accept stage's two table kernels (tally, then base + ident) over n_pairs pairs of host strings in
 * mhip_debug_push_gaps' layout, all alignments to one template: pair p starts at template position soff[p]; the base letters come from
 * tmpl_letters[tmpl_len].  Refused before anything runs: more than 255 pairs, a mismatch column, a pair whose template span leaves
 * [0, tmpl_len).  -> table_out[tmpl_len], ident_out[tmpl_len] */
int  mhip_debug_cns_table(mhip_ctx* ctx, const char* buf, int64_t bytes, const int64_t* off, const int32_t* len, const int32_t* soff,
                          int n_pairs, const char* tmpl_letters, int tmpl_len, mhip_cns_table_item* table_out, uint8_t* ident_out);
/* ---- mecat2cns' consensus plan, built in the accept stage behind the table (cns_plan.hip): what consensus_one_read_can_* decides from
 * the table alone.  Per template, with its read length L, the table, the ident bytes and the (soff, send) of its accepted alignments:
 *   effective ranges   tech 1: the one range (0, L) (mecat_correction.cpp:509; :357).  tech 0: get_effective_ranges (:118-153) — nothing
 *                      accepted: no range; an alignment with start <= 500 and L - end <= 500: the one range (0, L); otherwise the sweep over
 *                      the alignments sorted by (start asc, end desc), a range kept when right - left >= min_size * 0.95 (in double).  A
 *                      template without candidates has no table and no range.
 *   segments           consensus_worker (:203-239): inside every effective range, in order, each maximal run of positions with
 *                      mat_cnt + ins_cnt >= min_cov whose length satisfies end - beg >= 0.95 * min_size (in double).  A run does not
 *                      continue from one range into the next, even where they touch.
 *   windows            meap_consensus_one_segment (:81-108), inside a segment [beg, end): anchors are the positions with FMAT; from an
 *                      anchor i to the next anchor j (the segment's end if there is none) the window (sb = i, se = j) is listed when some
 *                      position of [i, j) has UNDS or FDEL — these are the stretches the reference hands to meap_cns_one_indel, with
 *                      cov = mat_cnt + ins_cnt at i as its min_cov (:103).  Positions in front of the first anchor belong to no window.
 * The mecat2cns defaults are min_cov 6 / min_size 5000 (PacBio) and 6 / 2000 (nanopore); min_size >= 2 and min_cov >= 1 are required.
 * Segments come in template order, then ascending beg: template t owns out_segments[out_seg_begin[t] .. out_seg_begin[t + 1]).  Windows
 * come in segment order, then ascending sb: segment s owns out_windows[win_begin .. win_end).  Effective ranges are (start, end) pairs:
 * template t owns pairs out_erange_begin[t] .. out_erange_begin[t + 1].  The output is the same bytes on every run.
 * mhip_cns_accept_templates_plan is mhip_cns_accept_templates_ex with MHIP_CNS_WANT_PLAN allowed in `want`: the plan needs the table, so
 * the table is built on the device whether or not MHIP_CNS_WANT_TABLE is set, but it is copied to the host only with that bit; with
 * MHIP_CNS_WANT_PLAN alone neither strings nor tables cross the PCIe link.  Without MHIP_CNS_WANT_PLAN the six plan outputs come back
 * NULL / 0 (their pointers may be NULL then) and min_cov / min_size are not looked at.  All buffers are released with mhip_cns_free.
 * Retrieving the windows' substrings: mhip_cns_accept_templates_pieces below; the POA: mhip_cns_accept_templates_poa; the corrected
 * reads: mhip_cns_accept_templates_reads. */
typedef struct { int32_t template_index, beg, end, n_anchors; int64_t win_begin, win_end; } mhip_cns_segment;
typedef struct { int32_t sb, se, cov, segment; } mhip_cns_window;       /* segment: index into out_segments */
#define MHIP_CNS_WANT_PLAN 4
int  mhip_cns_accept_templates_plan(mhip_ctx* ctx, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin,
                                    int num_templates, int tech, int min_align_size, double min_mapping_ratio, int num_threads, int want,
                                    int min_cov, int min_size, mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings,
                                    int64_t* out_strings_bytes, int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident,
                                    int64_t** out_table_begin /* [num_templates + 1] */, mhip_cns_segment** out_segments,
                                    int64_t** out_seg_begin /* [num_templates + 1] */, mhip_cns_window** out_windows, int64_t* out_n_windows,
                                    int32_t** out_eranges, int64_t** out_erange_begin /* [num_templates + 1] */);
/* test hook: the same host range function and the same plan kernels on host-supplied tables.  Template k owns table / ident
 * [table_begin[k], table_begin[k + 1]) and the mapping ranges (soff, send) ranges[2 r], ranges[2 r + 1] for r in [range_begin[k],
 * range_begin[k + 1]); both begin arrays have n_tmpl + 1 entries and start at 0.  The ident bytes are taken as given (they need not be
 * what the counts would give).  Refused: a mapping range that leaves its template.  Outputs as above. */
int  mhip_debug_cns_plan(mhip_ctx* ctx, const mhip_cns_table_item* table, const uint8_t* ident, const int64_t* table_begin, int n_tmpl,
                         const int32_t* ranges, const int64_t* range_begin, int tech, int min_cov, int min_size,
                         mhip_cns_segment** out_segments, int64_t** out_seg_begin, mhip_cns_window** out_windows, int64_t* out_n_windows,
                         int32_t** out_eranges, int64_t** out_erange_begin);
/* test hook: the plan's prefix-sum kernel — the single-workgroup scan every stage's count-to-position kernel calls (csrc/scan.h) — on a
 * host array: out[i] = base + cnt[0] + .. + cnt[i - 1] for i <= n, summed in 64 bits.  Refused before anything is launched: n < 0. */
int  mhip_debug_scan(mhip_ctx* ctx, const int32_t* cnt, int64_t n, int64_t base, int64_t* out /* [n + 1] */);
/* ---- the POA windows' substrings (cns_pieces.hip).  For a listed window (sb, se) the reference's meap_cns_one_indel
 * (mecat_correction.cpp:62-78) asks every accepted alignment of the template, in add order, for its part of the window:
 * CnsAln::retrieve_aln_subseqs (reads_correction_aux.h:47-68), a cursor per alignment that only moves forward, and feeds each pair of
 * substrings it gets to the graph with ag.addAln(qstr, tstr, sb_out - sb + 1).  A piece is one such answer as a descriptor: the
 * substrings are columns [col, col + ncols) of qaln and saln of accepted record `aln`, and sb_out = max(soff, sb).
 *   columns       column c >= 1 of an alignment has template position soff + the number of non-gap characters in saln[1 .. c]; column 0
 *                 has position soff whatever it holds (the cursor starts there without looking at it).
 *   a piece       runs from the first column at position max(soff, sb) to the first column at position se, gap columns in between
 *                 included, gap columns behind the base at se not; it stops at the last column, aln_size - 1, where the alignment ends
 *                 inside the window.
 *   no piece      se <= soff, sb >= send, aln_size < 2, or the template's previous listed window took the cursor to the last column
 *                 (it overlaps the alignment and its se lies on or behind the last column): an alignment whose last base is a window's
 *                 sb gives a one-column piece only when the stretch in front of that window was not listed.
 * mhip_cns_accept_templates_pieces is mhip_cns_accept_templates_plan with MHIP_CNS_WANT_PIECES allowed in `want`.  Window w of
 * out_windows owns out_pieces[out_piece_begin[w] .. out_piece_begin[w + 1]), in ascending `aln` — the reference's add order;
 * out_piece_begin has *out_n_windows + 1 entries ({0} when there is no window).  MHIP_CNS_WANT_PIECES needs MHIP_CNS_WANT_PLAN (refused
 * without it); PLAN | PIECES alone copies neither strings nor tables to the host.  Without the PIECES bit the call is
 * mhip_cns_accept_templates_plan (the two outputs come back NULL, their pointers may be NULL).  mhip_cns_accept_templates_plan and _ex
 * keep refusing the bit.  The output is the same bytes on every run; release with mhip_cns_free.  The POA itself (AlnGraphBoost):
 * mhip_cns_accept_templates_poa below. */
typedef struct { int32_t aln, col, ncols, sb_out; } mhip_cns_piece;   /* aln: index into out_accepted */
#define MHIP_CNS_WANT_PIECES 8
int  mhip_cns_accept_templates_pieces(mhip_ctx* ctx, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin,
                                      int num_templates, int tech, int min_align_size, double min_mapping_ratio, int num_threads, int want,
                                      int min_cov, int min_size, mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings,
                                      int64_t* out_strings_bytes, int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident,
                                      int64_t** out_table_begin /* [num_templates + 1] */, mhip_cns_segment** out_segments,
                                      int64_t** out_seg_begin /* [num_templates + 1] */, mhip_cns_window** out_windows, int64_t* out_n_windows,
                                      int32_t** out_eranges, int64_t** out_erange_begin /* [num_templates + 1] */,
                                      mhip_cns_piece** out_pieces, int64_t** out_piece_begin /* [*out_n_windows + 1] */);
/* test hook: the same piece kernels on ONE template: n_pairs alignments as host strings in mhip_debug_push_gaps' layout (pair p: qaln at
 * buf + off[p], len[p] characters + NUL, saln right behind it) with soff[p] / send[p], and n_windows listed windows windows[2 w] = sb,
 * windows[2 w + 1] = se.  `aln` of a piece is the pair's number.  Refused before anything is launched: more than 100 pairs
 * (MAX_CNS_OVLPS); len < 1; a pair outside the buffer; negative coordinates; a pair whose coordinates are not the ones add_aln would get
 * from the m5 record — [soff, send) is the stretch of template bases the strings hold, so send - soff must equal the number of non-gap
 * characters of saln[0 .. len) (for the usual saln[0] != '-': soff + 1 + the non-gap characters of saln[1 ..)); windows that are not
 * sb < se, not ascending or not disjoint (se of one > sb of the next).  -> *out_pieces, *out_piece_begin [n_windows + 1] */
int  mhip_debug_cns_pieces(mhip_ctx* ctx, const char* buf, int64_t bytes, const int64_t* off, const int32_t* len, const int32_t* soff,
                           const int32_t* send, int n_pairs, const int32_t* windows, int n_windows, mhip_cns_piece** out_pieces,
                           int64_t** out_piece_begin);
/* ---- the POA consensus of the listed windows (cns_poa.hip).  What the reference does with a listed window (sb, se, cov) is
 * meap_cns_one_indel (mecat_correction.cpp:62-78): an AlnGraphBoost over se - sb + 1 backbone positions (MECAT_AlnGraphBoost.C:76-97), one
 * addAln per piece with start = sb_out - sb + 1 (:99-152), mergeNodes (:219-357) and consensus((int)(cov * 0.4), cns) over bestPath
 * (:417-458, :508-592); meap_consensus_one_segment then appends cns without its first and last letter when it has more than two
 * (mecat_correction.cpp:104).  The device runs the same graph routine (csrc/cns_poa.h, pinned to the compiled reference by
 * tests/test_cns_poa_ref_cpu.py through its host build libcns_poa_host.so), one window per lane: windows whose workspace fits a slot of
 * mhip_cns_poa_small_words() 32-bit words in cns_poa_small, the others in cns_poa_large with workspaces of their own size, taken in
 * chunks of MECAT_CNS_POA_CHUNK_BYTES (default 1 GiB).  Every window is answered on the device.
 * mhip_cns_accept_templates_poa is mhip_cns_accept_templates_pieces with MHIP_CNS_WANT_POA allowed in `want`.  Window w of out_windows
 * owns the bytes out_cns[out_cns_begin[w] .. out_cns_begin[w + 1]) — `cns` as meap_cns_one_indel returns it, both end letters included,
 * no terminator; out_cns_begin has *out_n_windows + 1 entries ({0} when there is no window).  MHIP_CNS_WANT_POA needs
 * MHIP_CNS_WANT_PLAN (refused without it).  The pieces are computed on the device whenever the bit is set and copied to the host only
 * with MHIP_CNS_WANT_PIECES: PLAN | POA alone moves no strings, tables or pieces over the PCIe link.  Without the bit the call is
 * mhip_cns_accept_templates_pieces (the two outputs come back NULL, their pointers may be NULL).  _pieces, _plan and _ex keep refusing
 * the bit.  The output is the same bytes on every run; release with mhip_cns_free.  Putting the segments together from the windows'
 * strings (meap_consensus_one_segment's target) and the corrected reads: mhip_cns_accept_templates_reads below. */
#define MHIP_CNS_WANT_POA 16
int  mhip_cns_accept_templates_poa(mhip_ctx* ctx, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin,
                                   int num_templates, int tech, int min_align_size, double min_mapping_ratio, int num_threads, int want,
                                   int min_cov, int min_size, mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings,
                                   int64_t* out_strings_bytes, int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident,
                                   int64_t** out_table_begin /* [num_templates + 1] */, mhip_cns_segment** out_segments,
                                   int64_t** out_seg_begin /* [num_templates + 1] */, mhip_cns_window** out_windows, int64_t* out_n_windows,
                                   int32_t** out_eranges, int64_t** out_erange_begin /* [num_templates + 1] */,
                                   mhip_cns_piece** out_pieces, int64_t** out_piece_begin /* [*out_n_windows + 1] */,
                                   char** out_cns, int64_t** out_cns_begin /* [*out_n_windows + 1] */);
/* the slot of cns_poa_small in 32-bit words: a window goes there when 17 * nodes + 8 * edges <= this, with nodes = se - sb + 3 + the
 * insertion columns of its pieces (query letter over a template gap) and edges = se - sb + 2 + their match columns + their insertion
 * columns + the number of pieces */
int64_t mhip_cns_poa_small_words(void);
/* test hook: the piece kernels and then the POA kernels on ONE template: mhip_debug_cns_pieces' arguments, the windows as triples
 * windows[3 w] = sb, windows[3 w + 1] = se, windows[3 w + 2] = cov.  Refused before anything is launched: what mhip_debug_cns_pieces
 * refuses, and cov < 0.  -> *out_cns, *out_cns_begin [n_windows + 1] (malloc'ed, release with mhip_cns_free) */
int  mhip_debug_cns_poa(mhip_ctx* ctx, const char* buf, int64_t bytes, const int64_t* off, const int32_t* len, const int32_t* soff,
                        const int32_t* send, int n_pairs, const int32_t* windows, int n_windows, char** out_cns, int64_t** out_cns_begin);
/* test hook: the last POA launch of the process: out[0] = windows that went to cns_poa_large, out[1] = launches of it (chunks) */
void mhip_debug_cns_poa_last(int64_t* out /* [2] */);
/* ---- the corrected reads (cns_reads.hip): the rest of consensus_worker (mecat_correction.cpp:203-239), behind a slice's POA while its
 * table, plan and consensus strings are still in device memory.
 *   a segment's target   meap_consensus_one_segment, :88-107: positions of the segment [beg, end) in front of its first FMAT position give
 *                        nothing; from there every FMAT position i, ascending, gives table[i].base and, when the window with sb == i is
 *                        listed and its consensus has more than two letters, that string without its first and last letter.  The length
 *                        is n_anchors + the sum over the segment's windows of max(0, len - 2): lengths, the size filter and every output
 *                        position come from prefix sums before a letter is written.
 *   records              :233 and output_cns_result, :155-188: a target shorter than min_size gives nothing; one of at most 60 000 letters
 *                        gives one record with range (beg, end); a longer one is cut into blocks of 49 000 letters overlapping by 10 000,
 *                        the first block whose end reaches size - 11 000 ending at `size` (csrc/cns_reads.h: one function for the kernel
 *                        and for libcns_poa_host.so).  A block [L, R) has range_beg = L + beg and range_end = R + beg where R < size and
 *                        R + beg < end, otherwise end.  A target is stored once: the records of a cut segment point into overlapping
 *                        stretches of it, record r owning out_seq[seq_begin .. seq_begin + size).
 * read_id is the sid of the template's candidate records (what the reference passes as read_id), `segment` the batch-wide segment number
 * (the index into out_segments when those are copied).  Template t owns out_reads[out_read_begin[t] .. out_read_begin[t + 1]), in
 * segment order, then block order: the order in which consensus_worker pushes them for that template.
 * mhip_cns_accept_templates_reads is mhip_cns_accept_templates_poa with MHIP_CNS_WANT_READS allowed in `want`, alone or with any other
 * bit.  With the bit set the table, plan, pieces and POA are computed on the device whether or not their own bits are set, and each is
 * copied to the host only with its own bit: MHIP_CNS_WANT_READS alone moves the accepted records and the reads over the PCIe link, nothing
 * else (the outputs of the other bits come back NULL / 0).  min_cov and min_size are looked at (min_size >= 2, min_cov >= 1).
 * MHIP_CNS_WANT_PIECES and MHIP_CNS_WANT_POA keep needing MHIP_CNS_WANT_PLAN.  Without the bit the call is mhip_cns_accept_templates_poa,
 * byte for byte (the four outputs come back NULL / 0, their pointers may be NULL); _poa, _pieces, _plan and _ex keep refusing the bit.
 * The host waits once more per slice, for the two totals (letters, records) that size the output.  A flag word set by the kernels —
 * an index from the data left its array, or the letters written are not the letters counted — makes the call fail; nothing is
 * truncated.  The output is the same bytes on every run; out_read_begin has num_templates + 1 entries; release with mhip_cns_free. */
typedef struct { int32_t read_id, range_beg, range_end, size; int64_t seq_begin; int32_t template_index, segment; } mhip_cns_read;
#define MHIP_CNS_WANT_READS 32
int  mhip_cns_accept_templates_reads(mhip_ctx* ctx, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin,
                                     int num_templates, int tech, int min_align_size, double min_mapping_ratio, int num_threads, int want,
                                     int min_cov, int min_size, mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings,
                                     int64_t* out_strings_bytes, int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident,
                                     int64_t** out_table_begin /* [num_templates + 1] */, mhip_cns_segment** out_segments,
                                     int64_t** out_seg_begin /* [num_templates + 1] */, mhip_cns_window** out_windows, int64_t* out_n_windows,
                                     int32_t** out_eranges, int64_t** out_erange_begin /* [num_templates + 1] */,
                                     mhip_cns_piece** out_pieces, int64_t** out_piece_begin /* [*out_n_windows + 1] */,
                                     char** out_cns, int64_t** out_cns_begin /* [*out_n_windows + 1] */,
                                     mhip_cns_read** out_reads, int64_t** out_read_begin /* [num_templates + 1] */, char** out_seq,
                                     int64_t* out_seq_bytes);
/* The reference's text for n records (reads_correction_can.cpp:44-46): ">" read_id "_" range_beg "_" range_end "_" size, newline, the
 * letters, newline.  Host C++ only.  The two gates in front of the reference's loop (:32-33) need no code here: a template with fewer
 * than min_cov candidates cannot reach coverage min_cov anywhere, and a read shorter than 0.95 * min_size cannot hold a run of that
 * length, so neither can have a segment.  Refused: a record that leaves seq[0 .. seq_bytes).  -> *out_text (malloc'ed, no terminator,
 * release with mhip_cns_free), *out_bytes */
int  mhip_cns_format_reads(const mhip_cns_read* reads, int64_t n, const char* seq, int64_t seq_bytes, char** out_text, int64_t* out_bytes);
/* test hook: the read kernels alone on host-supplied arrays: tables and ident bytes of n_tmpl templates (template k at [table_begin[k],
 * table_begin[k + 1]), table_begin[0] == 0) with read ids read_id[k], n_seg segment records and n_win window records as the plan gives
 * them (numbers counted from 0, n_anchors as given), the windows' strings cns[cns_begin[w] .. cns_begin[w + 1]).  Refused before
 * anything is launched: min_size < 2; segments that are not in template order, a segment outside its template or not beg < end; segments
 * whose window ranges are not win_begin <= win_end, ascending and inside [0, n_win]; windows that are not sb < se, not ascending or not
 * disjoint inside their segment, that lie outside their segment or name another one; a cns_begin that does not start at 0 or does not
 * ascend.  What only the kernels can see (a window that does not start on an FMAT position, an n_anchors that is not the segment's) sets
 * the flag word: the call fails.  Outputs as mhip_cns_accept_templates_reads' four. */
int  mhip_debug_cns_reads(mhip_ctx* ctx, const mhip_cns_table_item* table, const uint8_t* ident, const int64_t* table_begin, int n_tmpl,
                          const int32_t* read_id, const mhip_cns_segment* segments, int64_t n_seg, const mhip_cns_window* windows,
                          int64_t n_win, const char* cns, const int64_t* cns_begin, int min_size, mhip_cns_read** out_reads,
                          int64_t** out_read_begin /* [n_tmpl + 1] */, char** out_seq, int64_t* out_seq_bytes);
/* test hook: the whole back end on ONE template through the launchers the accept stage uses — table, plan, pieces, POA, reads: the
 * alignments in mhip_debug_cns_pieces' layout, the template's letters (tmpl_len of them), tech (0: get_effective_ranges over the
 * alignments' (soff, send); 1: the whole read), min_cov, min_size and the read id.  Refused before anything is launched: what
 * mhip_debug_cns_table and mhip_debug_cns_pieces refuse (a mismatch column, a pair that leaves the template; more than 100 pairs,
 * len < 1, a pair outside the buffer, negative coordinates, send - soff != the bases of saln), min_size < 2, min_cov < 1.
 * -> *out_reads [*out_n_reads], *out_seq [*out_seq_bytes] (release with mhip_cns_free) */
int  mhip_debug_cns_correct(mhip_ctx* ctx, const char* buf, int64_t bytes, const int64_t* off, const int32_t* len, const int32_t* soff,
                            const int32_t* send, int n_pairs, const char* tmpl_letters, int tmpl_len, int tech, int min_cov, int min_size,
                            int read_id, mhip_cns_read** out_reads, int64_t* out_n_reads, char** out_seq, int64_t* out_seq_bytes);
/* ---- the corrected reads' FASTA text (cns_text.hip) and the entry point of the mecat2cns program (mecat_amd/cns/cns_main.cpp).
 * The text is the reference's (reads_correction_can.cpp:44-46; mhip_cns_format_reads above is the same text made on the host), made on
 * the device behind a slice's read kernels: a record's length is 1 + digits(read_id) + 1 + digits(range_beg) + 1 + digits(range_end) +
 * 1 + digits(size) + 1 + size + 1, the positions are a prefix sum, and a wave per record writes the header (lane l computes character l:
 * csrc/cns_text.h, one function for the kernel and for libcns_poa_host.so) and copies the letters with 16-byte stores.  A cut segment's
 * target is stored once on the device; the text repeats the overlapping stretches, so the duplication happens there and the host never
 * walks the output.  Records are in template order and slices hold whole templates: the slices' texts are concatenated as they are.
 * mhip_cns_correct_templates takes its options and outputs as structs instead of another 38 arguments:
 *   opts->tech, min_align_size, min_mapping_ratio, num_threads, min_cov, min_size   as in mhip_cns_accept_templates_reads
 *   opts->want          the MHIP_CNS_WANT_* bits, MHIP_CNS_WANT_TEXT among them
 *   opts->input_type    0: the walk of consensus_one_read_can_* (cands[] sorted by score in place, as in every entry point above).
 *                       1: the walk of consensus_one_read_m4_* (mecat_correction.cpp:241-360): a template's records are its overlaps, in
 *                       the order given.  With at most max_added of them (60 PacBio, 100 nanopore) every one is aligned, in that order;
 *                       with more, the template's range of cands[] is sorted in place with std::sort by max(qend - qoff, send - soff)
 *                       descending (CompareOverlapByOverlapSize, no tie-break: the same call on the same bytes gives the reference's
 *                       order) and the first max_added are aligned.  An overlap is accepted when GetAlignment succeeds and, for
 *                       nanopore only, check_ovlp_mapping_range with min_mapping_ratio - 0.02 holds; there is no used-ids set, no
 *                       coverage check and no limit of 200.  Everything behind the accept decisions is the same code.
 * With input_type 0 and `want` without MHIP_CNS_WANT_TEXT the call is mhip_cns_accept_templates_reads, byte for byte.  With
 * MHIP_CNS_WANT_TEXT the table, plan, pieces, POA and reads are computed on the device whether or not their bits are set, and each is
 * copied to the host only with its own bit: MHIP_CNS_WANT_TEXT alone moves the accepted records and the text over the PCIe link, nothing
 * else — in particular not the letters (out->seq stays NULL).  The host waits once more per slice, for the text's total.  The entry
 * points above keep refusing the bit.  Every member of *out is set (NULL / 0 where not asked for); release them with
 * mhip_cns_outputs_free, which leaves the struct zeroed (the members may also be released one by one with mhip_cns_free). */
#define MHIP_CNS_WANT_TEXT 64
typedef struct { int tech, input_type /* 0 .can walk, 1 m4 walk */, min_align_size, min_cov, min_size, num_threads, want; double min_mapping_ratio; } mhip_cns_opts;
typedef struct {
    mhip_cns_accepted* accepted; int64_t count; char* strings; int64_t strings_bytes; int64_t jobs;
    mhip_cns_table_item* table; uint8_t* ident; int64_t* table_begin /* [num_templates + 1] */;
    mhip_cns_segment* segments; int64_t* seg_begin /* [num_templates + 1] */; mhip_cns_window* windows; int64_t n_windows;
    int32_t* eranges; int64_t* erange_begin /* [num_templates + 1] */;
    mhip_cns_piece* pieces; int64_t* piece_begin /* [n_windows + 1] */;
    char* cns; int64_t* cns_begin /* [n_windows + 1] */;
    mhip_cns_read* reads; int64_t* read_begin /* [num_templates + 1] */; char* seq; int64_t seq_bytes;
    char* text; int64_t text_bytes;      /* no terminator */
} mhip_cns_outputs;
int  mhip_cns_correct_templates(mhip_ctx* ctx, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates,
                                const mhip_cns_opts* opts, mhip_cns_outputs* out);
void mhip_cns_outputs_free(mhip_cns_outputs* out);
/* test hook: the text kernels alone on n host-supplied records whose letters are seq[seq_begin .. seq_begin + size).  Refused before
 * anything is launched: a record that leaves seq[0 .. seq_bytes), a negative read_id, range_beg, range_end or size.
 * -> *out_text (malloc'ed, no terminator, release with mhip_cns_free), *out_bytes; n == 0 gives 0 bytes */
int  mhip_debug_cns_text(mhip_ctx* ctx, const mhip_cns_read* reads, int64_t n, const char* seq, int64_t seq_bytes, char** out_text, int64_t* out_bytes);
/* mhip_cns_free does not return a string buffer to the system at once: the library keeps the LARGEST released one (gigabytes — about
 * 14 GB for a config-2-sized batch) and hands it out again to the next batch that fits, because first-touching fresh pages costs
 * more than the batch's GPU time.  The parked buffer belongs to the process, not to a context (mhip_ctx_destroy leaves it).  This call
 * frees it; a process that is done with mecat2cns batches but lives on should call it. */
void mhip_cns_release_parked(void);

#ifdef __cplusplus
}
#endif
#endif
