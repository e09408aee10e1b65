// Recorder for tests/golden/make_golden_ref_rescue.py (build container only; nothing compiled from it is committed).  The generator
// compiles the reference's mecat2ref_aux.cpp, output.cpp and common sources where they lie into a temporary directory, weakens
// output_temp_result in output.o and links this main with them: it calls the UNMODIFIED rescue_clipped_align
// (mecat2ref/mecat2ref_aux.cpp:308-452) and output_results (:454-473) on hand-made AlignInfo arrays and hand-made segment records
// (Back_List) with a DiffAligner(0), as reference_mapping does (mecat2ref_impl_large.cpp:584-603), and records what they leave.  The
// output_temp_result defined here records WHICH result output_results prints instead of printing it.
//
// A second variant, compiled with -DREF_RESCUE_TOOL, is linked into the WHOLE unmodified mecat2ref instead (its own main): the generator
// renames rescue_clipped_align and output_results in mecat2ref_aux.o to orig_rescue_clipped_align / orig_output_results, and the two
// functions defined here under the tool's names record each call's arguments before and after (and the bytes output_results writes)
// around a call of the original.  Records go to the file $REF_RESCUE_OUT, int64:
//   {1, read, read_len, block_size, BC, naln before, nresults before, naln after, nresults after,
//    naln_before x {qoff, qend, qdir, soff, send, id}, naln_after x the nine fields below, nresults_after x the ten result fields below,
//    nevents, nevents x 8 words: what happened inside the call, in order —
//      {3, side (0 left / 1 right), CLIPPED gate failed on the read side, on the reference side, fill_clipped_candidate was called,
//       its block's score2, its return value, the search's return value}      one per find_left / find_right_clipped_candidate call
//      {4, loc1, loc2, score, chain, return value, 0, 0}                      one per extend_candidate call with alns == NULL}
// For these events the generator compiles a second copy of mecat2ref_aux.cpp as position-independent code (calls between its global
// functions then go through their symbols), weakens extend_candidate, fill_clipped_candidate and the two searches in the copy the tool
// uses, and keeps from the other copy only those four under the names orig_*: the functions of those names defined here record and
// call the originals.
//   {2, read, bytes written, crc32 of them, records}
//
// Input (argv[1]), int64 little-endian: ref_size, ncases; the reference's letters (upper-cased, one behind the other); per case
//   read_len, the read's letters, block_size, BC, num_output, naln, naln x {qoff, qend, qdir (0 'F' / 1 'R'), soff, send}, then for
//   the forward and for the reverse database: nseg, nseg x {segment, score2, loczhi[20], seedno[20]}.
// The first results (ids 0 .. naln - 1) have no strings; entry t of the given array has id t.
// Output (argv[2]), int64: per case
//   naln after, nresults after, naln_after x {qoff, qend, qdir, soff, send, id, prev_id, next_id, parent_id},
//   (nresults after - naln before) x {vscore, dir, qb, qe, qs, sb, se, cols, crc32(qmap), crc32(smap)},
//   nprinted, nprinted x id.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../common/diff_gapalign.h"
#include "../common/gapalign.h"
#include "mecat2ref_aux.h"
#include "output.h"

#define NENT 16          // AlignInfo alns[MAXC + 6] / TempResult results[MAXC + 6], mecat2ref_impl_large.cpp:311-313

static int64_t rd(FILE* f) {
    int64_t v;
    if (fread(&v, sizeof(v), 1, f) != 1) abort();
    return v;
}

static void wr(FILE* f, int64_t v) { fwrite(&v, sizeof(v), 1, f); }

static uint32_t crc32_of(const char* s, size_t n) {
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= (uint8_t)s[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

#ifndef REF_RESCUE_TOOL
static TempResult g_results[NENT];
static std::vector<int64_t> g_printed;

void output_temp_result(TempResult* result, FILE*) { g_printed.push_back((int64_t)(result - g_results)); }

static void read_db(FILE* in, std::vector<Back_List>& db) {
    std::fill(db.begin(), db.end(), Back_List());
    const int64_t nseg = rd(in);
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t seg = rd(in);
        if (seg < 0 || seg >= (int64_t)db.size()) abort();
        Back_List& b = db[(size_t)seg];
        memset(&b, 0, sizeof(b));
        b.score2 = (short)rd(in);
        b.score = b.score2;
        for (int i = 0; i < SM; ++i) b.loczhi[i] = (short)rd(in);
        for (int i = 0; i < SM; ++i) b.seedno[i] = (short)rd(in);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const int64_t ref_size = rd(in), ncases = rd(in);
    std::vector<char> ref((size_t)ref_size + 1, 0);
    if (fread(ref.data(), 1, (size_t)ref_size, in) != (size_t)ref_size) abort();
    DiffAligner* aligner = new DiffAligner(0);
    for (int i = 0; i < NENT; ++i) {
        memset(&g_results[i], 0, sizeof(TempResult));
        g_results[i].qmap = (char*)calloc(RM, 1);
        g_results[i].smap = (char*)calloc(RM, 1);
    }
    std::vector<Back_List> fwd_db((size_t)(ref_size / 1000 + 64)), rev_db(fwd_db.size());
    std::vector<char> qstr, tstr;
    for (int64_t ci = 0; ci < ncases; ++ci) {
        const int64_t L = rd(in);
        std::vector<char> fwd((size_t)L + 1, 0), rev;
        if (L && fread(fwd.data(), 1, (size_t)L, in) != (size_t)L) abort();
        rev = fwd;
        std::reverse(rev.begin(), rev.begin() + L);          // the strand as reference_mapping makes it (:374-408)
        for (int64_t j = 0; j < L; ++j) {
            char& c = rev[j];
            c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
        }
        const int block_size = (int)rd(in), bc = (int)rd(in), num_output = (int)rd(in);
        const int naln0 = (int)rd(in);
        if (naln0 > NENT - 6) abort();
        AlignInfo alns[NENT];
        memset(alns, 0, sizeof(alns));
        for (int t = 0; t < naln0; ++t) {
            AlignInfo& a = alns[t];
            a.qoff = (int)rd(in); a.qend = (int)rd(in); a.qdir = rd(in) ? 'R' : 'F'; a.soff = rd(in); a.send = rd(in);
            a.valid = 1; a.id = t; a.prev_id = a.next_id = a.parent_id = -1;
        }
        read_db(in, fwd_db);
        read_db(in, rev_db);
        int naln = naln0, nresults = naln0;
        rescue_clipped_align(alns, naln, g_results, nresults, aligner, ref.data(), ref_size, fwd.data(), rev.data(), qstr, tstr, (int)ci, (int)L, block_size, bc,
                             fwd_db.data(), rev_db.data(), 0.25);
        g_printed.clear();
        int naln_o = naln, nres_o = nresults;
        output_results(alns, naln_o, g_results, nres_o, num_output, NULL);
        if (naln_o != naln || nres_o != nresults) abort();
        wr(out, naln); wr(out, nresults);
        for (int t = 0; t < naln; ++t) {
            const AlignInfo& a = alns[t];
            wr(out, a.qoff); wr(out, a.qend); wr(out, a.qdir == 'R'); wr(out, a.soff); wr(out, a.send); wr(out, a.id); wr(out, a.prev_id); wr(out, a.next_id);
            wr(out, a.parent_id);
        }
        for (int t = naln0; t < nresults; ++t) {
            const TempResult& r = g_results[t];
            const size_t cols = strlen(r.qmap);
            if (strlen(r.smap) != cols) abort();
            wr(out, r.vscore); wr(out, r.read_dir == 'R'); wr(out, r.qb); wr(out, r.qe); wr(out, r.qs); wr(out, r.sb); wr(out, r.se); wr(out, (int64_t)cols);
            wr(out, crc32_of(r.qmap, cols)); wr(out, crc32_of(r.smap, cols));
        }
        wr(out, (int64_t)g_printed.size());
        for (size_t t = 0; t < g_printed.size(); ++t) wr(out, g_printed[t]);
    }
    fclose(out);
    return 0;
}

#else  // REF_RESCUE_TOOL

extern "C" void orig_rescue_clipped_align(AlignInfo* alnv, int& naln, TempResult* results, int& nresults, GapAligner* aligner, const char* raw_ref, const long ref_size,
                                          const char* fwd_raw_read, const char* rev_raw_read, std::vector<char>& qstr, std::vector<char>& tstr, int read_name,
                                          int read_len, int block_size, int BC, Back_List* fwd_database, Back_List* rev_database, double ddfs_cutoff);
extern "C" void orig_output_results(AlignInfo* alnv, int& naln, TempResult* results, int& nresults, int num_output, FILE* out);

extern "C" bool orig_extend_candidate(candidate_save& can, GapAligner* aligner, const char* raw_ref, const long ref_size, const char* fwd_raw_read, const char* rev_raw_read,
                                      std::vector<char>& qstr, std::vector<char>& tstr, int read_name, int read_len, AlignInfo* alns, int* naln, TempResult* trv, int& ntr);
extern "C" bool orig_fill_clipped_candidate(Back_List* block, long bid, candidate_save& can, char chain, int read_size, int BC, int block_size, double ddfs_cutoff);
extern "C" bool orig_find_left_clipped_candidate(AlignInfo& aln, candidate_save& can, Back_List* database, int block_size, int read_size, int BC, double ddfs_cutoff);
extern "C" bool orig_find_right_clipped_candidate(AlignInfo& aln, candidate_save& can, Back_List* database, int block_size, int read_size, long ref_size, int BC,
                                                  double ddfs_cutoff);

static FILE* g_rec = NULL;
static int g_read = -1;
static std::vector<int64_t> g_events;
static int64_t g_fill[3] = {0, 0, 0};          // called, score2, return value of the search in hand

bool extend_candidate(candidate_save& can, GapAligner* aligner, const char* raw_ref, const long ref_size, const char* fwd_raw_read, const char* rev_raw_read,
                      std::vector<char>& qstr, std::vector<char>& tstr, int read_name, int read_len, AlignInfo* alns, int* naln, TempResult* trv, int& ntr) {
    const bool r = orig_extend_candidate(can, aligner, raw_ref, ref_size, fwd_raw_read, rev_raw_read, qstr, tstr, read_name, read_len, alns, naln, trv, ntr);
    if (!alns) {
        const int64_t v[8] = {4, can.loc1, can.loc2, can.score, can.chain == 'R', r, 0, 0};
        g_events.insert(g_events.end(), v, v + 8);
    }
    return r;
}

bool fill_clipped_candidate(Back_List* block, long bid, candidate_save& can, char chain, int read_size, int BC, int block_size, double ddfs_cutoff) {
    const bool r = orig_fill_clipped_candidate(block, bid, can, chain, read_size, BC, block_size, ddfs_cutoff);
    g_fill[0] = 1; g_fill[1] = block->score2; g_fill[2] = r;
    return r;
}

bool find_left_clipped_candidate(AlignInfo& aln, candidate_save& can, Back_List* database, int block_size, int read_size, int BC, double ddfs_cutoff) {
    g_fill[0] = g_fill[1] = g_fill[2] = 0;
    const bool r = orig_find_left_clipped_candidate(aln, can, database, block_size, read_size, BC, ddfs_cutoff);
    const int64_t v[8] = {3, 0, aln.qoff <= CLIPPED, aln.soff <= CLIPPED, g_fill[0], g_fill[1], g_fill[2], r};
    g_events.insert(g_events.end(), v, v + 8);
    return r;
}

bool find_right_clipped_candidate(AlignInfo& aln, candidate_save& can, Back_List* database, int block_size, int read_size, long ref_size, int BC, double ddfs_cutoff) {
    g_fill[0] = g_fill[1] = g_fill[2] = 0;
    const bool r = orig_find_right_clipped_candidate(aln, can, database, block_size, read_size, ref_size, BC, ddfs_cutoff);
    const int64_t v[8] = {3, 1, read_size - aln.qend <= CLIPPED, ref_size - aln.send <= CLIPPED, g_fill[0], g_fill[1], g_fill[2], r};
    g_events.insert(g_events.end(), v, v + 8);
    return r;
}

static FILE* rec_file() {
    if (!g_rec) {
        const char* p = getenv("REF_RESCUE_OUT");
        if (!p || !(g_rec = fopen(p, "wb"))) abort();
    }
    return g_rec;
}

void rescue_clipped_align(AlignInfo* alnv, int& naln, TempResult* results, int& nresults, GapAligner* aligner, const char* raw_ref, const long ref_size,
                          const char* fwd_raw_read, const char* rev_raw_read, std::vector<char>& qstr, std::vector<char>& tstr, int read_name, int read_len,
                          int block_size, int BC, Back_List* fwd_database, Back_List* rev_database, double ddfs_cutoff) {
    FILE* f = rec_file();
    const int naln0 = naln, nres0 = nresults;
    std::vector<int64_t> before;
    for (int t = 0; t < naln0; ++t) {
        const AlignInfo& a = alnv[t];
        const int64_t v[6] = {a.qoff, a.qend, a.qdir == 'R', a.soff, a.send, a.id};
        before.insert(before.end(), v, v + 6);
    }
    g_events.clear();
    orig_rescue_clipped_align(alnv, naln, results, nresults, aligner, raw_ref, ref_size, fwd_raw_read, rev_raw_read, qstr, tstr, read_name, read_len, block_size, BC,
                              fwd_database, rev_database, ddfs_cutoff);
    g_read = read_name;
    wr(f, 1); wr(f, read_name); wr(f, read_len); wr(f, block_size); wr(f, BC); wr(f, naln0); wr(f, nres0); wr(f, naln); wr(f, nresults);
    for (size_t i = 0; i < before.size(); ++i) wr(f, before[i]);
    for (int t = 0; t < naln; ++t) {
        const AlignInfo& a = alnv[t];
        wr(f, a.qoff); wr(f, a.qend); wr(f, a.qdir == 'R'); wr(f, a.soff); wr(f, a.send); wr(f, a.id); wr(f, a.prev_id); wr(f, a.next_id); wr(f, a.parent_id);
    }
    for (int t = 0; t < nresults; ++t) {
        const TempResult& r = results[t];
        const size_t cols = strlen(r.qmap);
        if (strlen(r.smap) != cols) abort();
        wr(f, r.vscore); wr(f, r.read_dir == 'R'); wr(f, r.qb); wr(f, r.qe); wr(f, r.qs); wr(f, r.sb); wr(f, r.se); wr(f, (int64_t)cols);
        wr(f, crc32_of(r.qmap, cols)); wr(f, crc32_of(r.smap, cols));
    }
    wr(f, (int64_t)(g_events.size() / 8));
    for (size_t i = 0; i < g_events.size(); ++i) wr(f, g_events[i]);
    fflush(f);
}

void output_results(AlignInfo* alnv, int& naln, TempResult* results, int& nresults, int num_output, FILE* out) {
    FILE* f = rec_file();
    char* buf = NULL;
    size_t len = 0;
    FILE* mem = open_memstream(&buf, &len);
    orig_output_results(alnv, naln, results, nresults, num_output, mem);
    fclose(mem);
    int64_t lines = 0;
    for (size_t i = 0; i < len; ++i) lines += buf[i] == '\n';
    wr(f, 2); wr(f, g_read); wr(f, (int64_t)len); wr(f, crc32_of(buf, len)); wr(f, lines / 3);
    fwrite(buf, 1, len, out);
    free(buf);
    fflush(f);
}

#endif
