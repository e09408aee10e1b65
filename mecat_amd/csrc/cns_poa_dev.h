// cns_poa_dev.h — the POA kernels' launch (cns_poa.hip), used by cns_accept.hip behind a slice's pieces
#pragma once
#include "common.h"
#include "cns_pieces.h"

// words of a window's slot in cns_poa_small (cns_poa_words(nodes, edges) of cns_poa.h): 16 KiB.  The slots of the resident lanes — two
// blocks of 256 per CU — then take 2 GiB at 256 CUs; a window of 20 positions with 10 pieces of 25 columns (some 60 nodes, 290 edges:
// 3 340 words) fits, a nanopore window with 100 pieces does not and goes to cns_poa_large.
#define CNS_POA_SLOT_WORDS 4096

struct CnsPoaDev {
    const char* d_cns = nullptr;            // [cap] bytes; the first d_cb[nwin] are the windows' strings, no terminators
    const long long* d_cb = nullptr;        // [nwin + 1] first byte of every window's string, counted from the launch's first
    const long long* d_bad = nullptr;       // nonzero once the kernels have run: the routine returned a code, or an index left its array
    long long cap = 0;                      // the bound the buffers were sized by: sum over the windows of (nodes - 2)
    long long nlarge = 0;                   // windows that went to cns_poa_large, and the launches (chunks) that took
    int nchunks = 0;
    double wait_s = 0;                      // host seconds spent in the wait for the bounds
};

// The consensus of `nwin` windows d_win[] from their pieces `pd` (cns_pieces_launch's output for the same windows, strings d_str, `na`
// alignments, records' aln counted from aln_base).  Everything runs on c->stream; the function WAITS for the stream once and returns
// with the last kernel launched.  `set` (0 / 1) picks the scratch buffers: the arrays behind `out` stay valid until the next call
// with the same set.
int cns_poa_launch(mhip_ctx* c, int set, const char* d_str, const CnsPiecesDev& pd, long long na, long long aln_base, const mhip_cns_window* d_win, long long nwin,
                   CnsPoaDev* out);
