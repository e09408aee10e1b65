// ref_reads.h — query reads as the volume mecat2ref's stages map.
//
// mecat2ref does not upper-case reads, and its two stages read a letter differently:
//   seeding     atcttrans (mecat2ref_impl_large.cpp:44-51) knows upper-case A, C, G, T only: a k-mer with any other letter is skipped
//   extension   extract_sequences (mecat2ref_aux.cpp:114-120) encodes with get_dna_encode_table (common/defs.cpp:3-33), which knows lower
//               case too: a, c, g, t are 0..3, every other letter is 0; and the reverse strand is the whole read reversed with only
//               upper-case A, C, G, T complemented (mecat2ref_impl_large.cpp:376-410)
// Hence the packing: pac holds the extension's code of every letter (lower-case a, c, g, t as 0..3, other letters 0), nplane is 3 at
// every letter that is not an upper-case A, C, G or T.  ref_seed.hip skips a k-mer on the plane alone; ref_extend.hip keeps the stored
// code of a base on the plane when it takes the reverse strand and complements the others.  Layout: the volume ABI's (first base in
// the two top bits of a byte, one pad base behind every read).
#pragma once
#include <stdint.h>

#include <vector>

#include "mecat_hip.h"

struct RefReads {
    int64_t num_bases = 0;                 // incl. one pad base per read
    std::vector<uint8_t> pac, nplane;      // (num_bases + 3) / 4 bytes each
    std::vector<mhip_offset_t> reads;
};

// the letters of n reads -> r; false when the reads do not fit one volume (int32 positions)
bool ref_reads_pack(const char* const* seqs, const int* lens, int n, RefReads* r);
// the volume with its N plane; 0, or non-zero with the message in mhip_last_error()
int ref_reads_upload(mhip_ctx* ctx, const RefReads& r, mhip_volume** vol);
