// ref_results.h — a result of mhip_ref_extend_fetch as the text and records mecat2ref's later stages consume (stages 2
// and 3).  No HIP.
//
// Replaces, behind DiffAligner::go (common/diff_gapalign.cpp:309-346: the two strings over "ACGT-"):
//   extend_candidate    mecat2ref/mecat2ref_aux.cpp:154-177   the TempResult's strings and the AlignInfo entry
//   output_temp_result  mecat2ref/output.cpp:238-252          the record of the temporary result files
//   output_results      mecat2ref/mecat2ref_aux.cpp:454-473   a read's records in the order mhip_ref_rescue_fetch's out_slots names them
// The device hands over coordinates and 2-bit columns in string order (0 = both bases, 1 = target base only, 2 = query base only); the
// letters come from the two packed sequences in one forward walk: the query from (qb, strand) of the read as ref_reads.h packs it, the
// target from base sb of the reference volume (ref_genome.h).
#pragma once
#include <stdint.h>

#include <string>

#include "mecat_hip.h"

// AlignInfo as extend_candidate fills it (mecat2ref_aux.h:9-20, mecat2ref_aux.cpp:166-177); qid is not set there
struct RefAlignInfo {
    int qid = 0, qoff = 0, qend = 0;
    int parent_id = -1, id = 0, prev_id = -1, next_id = -1;
    char valid = 1;
    char qdir = 'F';
    long soff = 0, send = 0;
};

// code (0..3) of base `idx` of a packed plane (first base in the two top bits of a byte)
inline int ref_packed_code(const uint8_t* pac, int64_t idx) { return (pac[idx >> 2] >> ((~idx & 3) << 1)) & 3; }

// qmap / smap of result r: cols = its words of ops_dense, read_off = the read's offset in the reads volume (mhip_offset_t::offset).
// false when the columns do not add up to the result's coordinates (a damaged hand-over).
bool ref_result_strings(const mhip_ref_result& r, const uint32_t* cols, const uint8_t* reads_pac, const uint8_t* reads_nplane, int64_t read_off,
                        const uint8_t* ref_pac, std::string* qmap, std::string* smap);
// the bytes output_temp_result writes
std::string ref_result_record(int read_id, const mhip_ref_result& r, const std::string& qmap, const std::string& smap);
// the entry extend_candidate appends for the read's result number `id` (its index in the read's result list)
RefAlignInfo ref_result_align_info(const mhip_ref_result& r, int id);

// One set of extension results of one read: its rows of a fetch's res, and where their columns lie (word_offs + the read's first slot
// and the whole ops_dense array: result k occupies words [offs[k], offs[k + 1]) of `words`)
struct RefResultSet {
    const mhip_ref_result* res = nullptr;
    const uint64_t* offs = nullptr;
    const uint32_t* words = nullptr;
    int count = 0;          // slots of the read in this set: maxc for the first extension, 6 for the rescue
};
// The bytes output_results writes for one read into the per-thread result file: the records of out_slots[0 .. out_count) in that order
// (slot s < first.count = the first extension's slot s, else rescue slot s - first.count).  false when a slot names no ok result or its
// columns do not add up.
bool ref_read_records(int read_id, const int32_t* out_slots, int out_count, const RefResultSet& first, const RefResultSet& rescue,
                      const uint8_t* reads_pac, const uint8_t* reads_nplane, int64_t read_off, const uint8_t* ref_pac, std::string* out);
