// pw_row.h — one grid row of mecat2pw (pw_row.cpp)
#pragma once

#include <stdio.h>

#include <string>
#include <vector>

#include "mecat_hip.h"
#include "options.h"

class PartitionWriter;

// Reference volume `svid` against the query volumes svid .. V - 1; the lines go to `out`, their records to `pw` (may be NULL).
// comm == NULL: this process computes the whole grid row.  Otherwise every rank of the communicator runs this function for the
// same row: the reads of a slab are dealt out in chunks (chunk c of query volume j -> rank (c + j) mod P), each rank seeds and
// extends its own, the lists are all-gathered (mhip_seed_reads_sharded / mhip_align_sharded), and every rank formats and writes the
// lines of its own reads into its part of r_<i> (out = that part).
void process_one_volume(const Options& opt, mhip_ctx* ctx, int svid, const std::vector<std::string>& vn, FILE* out, PartitionWriter* pw,
                        double part_ratio, mhip_comm* comm, int shard_chunk);
