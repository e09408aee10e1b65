// ref_genome.h — a reference FASTA file as the volume mecat2ref's index is built from (stage 1).
//
// Replaces creat_ref_index's reading of the reference file (mecat2ref/mecat2ref_impl_large.cpp:152-184): the letters of all records
// one behind the other with nothing between chromosomes, '\n' and '\r' skipped, a letter above 'Z' upper-cased, the name = the header
// up to its first space or tab, and the text of chrindex.txt.  From the letters:
//   pac      the 2-bit store of the volume ABI (A, C, G, T = 0..3; every other letter stored as 0)
//   nplane   3 at every letter that is not A, C, G, T (mhip_volume_set_nplane's layout)
//   reads    the volume's read table: the maximal runs of A, C, G, T.  mhip_index_build starts no 13-mer at the 13 positions that end at
//            a read's end ([end - 12, end]), which is every 13-mer that holds the letter behind a run.  It knows nothing about the
//            space BETWEEN reads, so a longer stretch of other letters gets zero-length reads no more than 13 apart, the last one on the
//            stretch's last letter: together they mark exactly the 13-mers that hold such a letter (creat_ref_index restarts its
//            k-mer there, :194-199).  A k-mer across two chromosomes is kept, as there.
// Positions are int32 in the volume ABI: a reference that does not fit one volume is refused with a message.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "mecat_hip.h"

struct RefChrom {
    int64_t start = 0, size = 0;
    std::string name;
};

struct RefGenome {
    int64_t num_bases = 0;
    std::vector<uint8_t> pac, nplane;      // (num_bases + 3) / 4 bytes each
    std::vector<mhip_offset_t> reads;
    std::vector<RefChrom> chroms;
    std::string chrindex;                  // the bytes of chrindex.txt: `start \t name \t size` per record, then `count \t FileEnd`
};

// the file's bytes -> g; false with *err set when the text is no FASTA file or does not fit one volume
bool ref_genome_parse(const char* text, size_t n, RefGenome* g, std::string* err);
bool ref_genome_load(const char* path, RefGenome* g, std::string* err);
// the volume (with its N plane) and its index (plain mhip_index_build); 0, or non-zero with the message in mhip_last_error()
int ref_genome_upload(mhip_ctx* ctx, const RefGenome& g, mhip_volume** vol, mhip_index** idx);
