// cns_pieces.h — the POA windows' substrings as descriptors (CnsAln::retrieve_aln_subseqs on the device, cns_pieces.hip), used by
// cns_accept.hip behind a slice's plan
#pragma once
#include "common.h"

struct CnsPieceItem {
    unsigned long long off;      // byte offset of the query string in the string buffer; the template string follows at off + aln_size + 1
    int32_t aln_size;            // columns
    int32_t soff, send;          // m5soff / m5send, what add_aln gets
    int32_t tl;                  // the alignment's template, counted from the launch's first one
};

struct CnsPiecesDev {
    const mhip_cns_piece* d_pieces = nullptr;     // [cap] slots; the first d_pb[nwin] hold the records, final (global `aln`)
    const long long* d_pb = nullptr;              // [nwin + 1] first piece of every window, counted from the launch's first piece
    const CnsPieceItem* d_items = nullptr;        // [na] the launch's items[] on the device (what cns_poa.hip finds a piece's strings with)
    const long long* d_bad = nullptr;             // nonzero once the kernels have run: an index derived from the data left its array (NULL: nothing ran)
    long long cap = 0;                            // the bound on the pieces the buffers were sized by: sum over the alignments of the windows they overlap
    double wait_s = 0;                            // host seconds spent in the wait for that bound
};

// The pieces of `nwin` windows d_win[] (the launch's part of a plan, in plan order: window records with global segment numbers from
// seg_base, d_seg[nseg] their segments with global window numbers from win_base, d_segb[nt + 1] the templates' first segments) over `na`
// alignments whose strings lie in d_str.  items[na] (template after template: template k owns [afirst[k], afirst[k + 1])), afirst[nt + 1]
// and tb[nt + 1] (template k has tb[k + 1] - tb[k] positions) are HOST arrays.  Everything runs on c->stream behind what the stream
// holds; the function WAITS for the stream once (the bound on the pieces sizes their buffers) and returns with the last kernel
// launched.  `set` (0 / 1) picks the scratch buffers: the arrays behind `out` stay valid until the next call with the same set.
// Records come out final: aln = aln_base + the alignment's index in items[].
int cns_pieces_launch(mhip_ctx* c, int set, const char* d_str, const CnsPieceItem* items, long long na, long long aln_base, int nt, int t_index0,
                      const long long* afirst, const long long* tb, const mhip_cns_segment* d_seg, long long nseg, const long long* d_segb, long long seg_base,
                      long long win_base, const mhip_cns_window* d_win, long long nwin, CnsPiecesDev* out);

// The front half of the test hooks mhip_debug_cns_pieces and mhip_debug_cns_poa: ONE template's alignments as host strings (see
// mecat_hip.h) and n_windows windows of `wstride` ints each — (sb, se) or (sb, se, cov) — checked, uploaded and run through
// cns_pieces_launch (set 0).  n_windows == 0 launches nothing and leaves *pd empty.  *d_buf: the strings on the device, *d_win the
// window records (cov 0 with wstride 2); both are scratch of `c`.
int cns_pieces_debug_launch(mhip_ctx* c, const char* buf, int64_t bytes, const int64_t* off, const int32_t* len, const int32_t* soff, const int32_t* send, int n_pairs,
                            const int32_t* windows, int wstride, int n_windows, CnsPiecesDev* pd, const char** d_buf, const mhip_cns_window** d_win);
