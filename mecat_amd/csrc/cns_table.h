// cns_table.h — mecat2cns' consensus table of accepted alignments, tallied on the device (cns_table.hip), used by cns_accept.hip
#pragma once
#include "common.h"

struct CnsTabItem {
    unsigned long long off;      // byte offset of the query string in the string buffer; the template string follows at off + aln_size + 1
    unsigned long long tab;      // word offset of the template's table in the table buffer
    int32_t aln_size;            // columns
    int32_t soff;                // template position of the first template base of the strings (m5soff)
    int32_t tab_len;             // positions of that table (bases of the template read): nothing is added outside [0, tab_len)
    int32_t pad;
};

// One 32-bit word per template position, bytes {base, mat_cnt, ins_cnt, del_cnt} from the least significant one (mhip_cns_table_item).
// cns_table_launch zeroes d_table[0 .. n_words), tallies the n_items alignments whose strings lie in d_str into it, then writes every
// word's base byte and d_ident[0 .. n_words).  The letter of a position comes from `d_letters` (one template: position w has letter
// d_letters[w]) when that is not NULL, else from the volume: table words [d_first[k], d_first[k + 1]) belong to a read whose base 0 is
// volume base d_voloff[k], k < n_tmpl.  Everything on c->stream, waits for nothing; the host arrays behind the device arrays handed in
// are the caller's to keep alive.
int cns_table_launch(mhip_ctx* c, const mhip_volume* vol, const char* d_str, const CnsTabItem* d_items, int n_items, uint32_t* d_table, uint8_t* d_ident,
                     long long n_words, const long long* d_first, const int32_t* d_voloff, int n_tmpl, const char* d_letters);
