// pw_run.h — the multi-process protocol of mecat2pw: P processes, one per GPU, whose hand-offs are files in the working directory.
//
// Multi-GPU mode (additive): P processes, one per GPU, started with WORLD_SIZE / RANK / LOCAL_RANK in the environment (e.g.
// `python -m torch.distributed.run --no-python --nproc-per-node 8 mecat2pw ...`) or MECAT_HIP_WORLD / MECAT_HIP_RANK.  Rank 0
// splits the input, merges the r_<i> files and writes the output; hand-offs between the processes are files in wrk_dir, like
// the resume protocol itself.  Two ways to share the volume x volume grid (MECAT_HIP_SHARD=rows|cells overrides the choice):
//   rows   (#volumes >= P)  the grid rows still to do are dealt out by cost (row i = num_vols - i cells, heaviest first to the least
//          loaded rank: mhip_shard_deal_rows), each row computed by one GPU exactly as in a single-GPU run (one index build per row, no
//          data moves between the processes);
//   cells  (#volumes <  P)  every rank works on every cell: the query reads of a cell are dealt out in chunks of 500
//          (MECAT_HIP_SHARD_CHUNK; chunk c of query volume j -> rank (c + j) mod P), each rank builds the index of
//          the row's reference volume itself, and the candidate lists / extension results are all-gathered over RCCL
//          (mhip_seed_reads_sharded, mhip_align_sharded); every rank formats and writes the lines of its own reads (r_<i>.part<rank>),
//          rank 0 strings the parts together into r_<i>.  A one-volume input (config 2) uses every GPU.
// A run is identified by a token (MECAT_HIP_RUN_ID, else the launcher's TORCHELASTIC_RUN_ID + the parent pid, which every rank
// of one launch shares): rank 0 puts it into the split marker, the other ranks accept no other marker.  Every rank keeps a
// heartbeat file fresh and leaves a failure marker when it aborts; rank 0 stops waiting for a row whose owner has died.
#pragma once

#include <stdint.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "mecat_hip.h"

struct RunFiles {
    std::string dir, token;
    std::string marker() const { return dir + "split_done"; }
    std::string alive(int r) const { return dir + "rank_" + std::to_string(r) + ".alive." + token; }
    std::string failed(int r) const { return dir + "rank_" + std::to_string(r) + ".failed." + token; }
};

struct Run {
    int world = 1, rank = 0;
    double t_start = 0;
    RunFiles rf;
    bool explicit_token = false;      // MECAT_HIP_RUN_ID was given
    double wait_limit = 0;            // MECAT_HIP_WAIT_S: patience with the other ranks' files
};
Run run_from_env(const char* wrk_dir);

// what rank 0 decides after the split and every rank works from
struct Split {
    int num_vols = 0;
    bool cells = false;
    std::vector<int> todo;                         // grid rows this run still has to compute
    uint8_t comm_id[MHIP_COMM_ID_BYTES] = {0};
};
void publish_split(const Run& run, const Split& s);                    // rank 0: the split marker, complete or not at all
void await_split(const Run& run, const char* wrk_dir, Split* s);       // the other ranks: wait for THIS run's marker

// Is the failure marker of rank `peer` there, and to be believed (the stale-marker rule, pw_run.cpp)?
bool peer_failed(const Run& run, int peer);

// heartbeat + failure marker of every rank of a multi-process run, and a watchdog on the peers: a rank that sees another
// rank's failure marker (or, once that rank's heartbeat has been seen, no beat for a minute) leaves its own marker and exits —
// also when its main thread sits inside an RCCL collective the dead rank will never join (cells mode had no timeout)
class Heartbeat {
public:
    void start(const Run& run);      // (nothing in a one-process run)
    void stop();                     // stops and joins the thread, which removes its heartbeat file itself
    ~Heartbeat() { stop(); }

private:
    std::atomic<bool> stop_{false};
    std::thread t_;
};

// rank 0, rows mode: returns when `fin` (row i, computed by `owner`) is there; dies when the owner has
void wait_for_row(const Run& run, const std::string& fin, int owner, int i);
// rank 0: returns when rank r's partition streams are complete (`meta` is there)
void wait_for_partition_streams(const Run& run, const std::string& meta, int r, double w0);
