// Recorder for tests/golden/make_golden_ref_xext.py (build container only; nothing compiled from it is committed).  The generator compiles
// the reference's mecat2ref_aux.cpp, output.cpp and common sources where they lie into a temporary directory and links this main with
// them: it calls the UNMODIFIED extend_candidate (mecat2ref/mecat2ref_aux.cpp:123-183) with an XdropAligner(0), as reference_mapping does
// in nanopore mode (mecat2ref_impl_large.cpp:328-335), once per given candidate, and records what the aligner holds afterwards.
//
// Input (argv[1]), int64 little-endian: ref_size, nreads, ncand; the reference's letters as the tool holds them (one behind the other,
// upper-cased); per read its length and letters; per candidate {read, chain (0 'F' / 1 'R'), loc1, loc2, score}.
// The reverse strand is made the way reference_mapping makes it (:374-408): the read reversed, upper-case A, C, G, T complemented.
// Output argv[2]: per candidate 21 int64
//   {ok, qb, qe, qs, ts, te, cols, lraw, rraw, sb, se, matches,  L: blocks, sized_last, xdrop_end, failed_trim,  R: the same four,  ns}
//   ts / te = the aligner's target_start / target_end inside the window; sb / se = the TempResult's (ok results only);
//   lraw / rraw = the columns of the two halves as align_ex leaves them (go joins the left one without its last column, :401-402);
//   matches = the columns of the joined strings with equal letters; ns = nanoseconds of the extend_candidate call.
// The per-direction facts come from a second pass over the same sequences that chains the reference's own retrieve_next_aln_block,
// xdrop_align, script_to_aligned_string and trim_mismatch_end the way align_ex does (xdrop_gapalign.cpp:263-357) and must arrive at the
// same number of columns:
//   blocks       blocks aligned;  sized_last = the last block was cut by the `x 1.2` rule (gapalign.cpp:26-29), not by what was left
//   xdrop_end    the direction ended in a block that stopped more than 20 bases before both of its ends (!full_map): the X-drop
//   failed_trim  the direction ended because trim_mismatch_end found no tail to anchor on (the block's columns are dropped)
// Output argv[3]: per candidate int64 cols, then the query string and the target string (cols bytes each).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../common/gapalign.h"
#include "../common/xdrop_gapalign.h"
#include "mecat2ref_aux.h"
#include "output.h"

int xdrop_align(const char* A, const int M, const char* B, const int N, int matrix[][4], int gap_open, int gap_extend, int x_dropoff, u8* state_array,
                BlastGapDP* score_array, u8** edit_script, int* edit_start_offset, GapPrelimEditBlock* edit_block, const bool forward, int& ae, int& be);
void script_to_aligned_string(const char* query, const char* target, int qe, int te, GapPrelimEditBlock* edit_block, const bool forward, std::string& qaln,
                              std::string& taln);

static int64_t rd(FILE* f) {
    int64_t v;
    if (fread(&v, sizeof(v), 1, f) != 1) abort();
    return v;
}

struct DirFacts { int64_t blocks, sized_last, xdrop_end, failed_trim, cols; };

static DirFacts probe(XdropAligner* a, const char* query, const int query_size, const char* target, const int target_size, const bool forward) {
    DirFacts F = {0, 0, 0, 0, 0};
    int qidx = 0, tidx = 0, qblk, tblk, qe, te;
    const char *Q, *T;
    std::string tq, tt;
    while (1) {
        const bool last = retrieve_next_aln_block(query, qidx, query_size, target, tidx, target_size, a->param.block_size, forward, Q, T, qblk, tblk);
        xdrop_align(Q, qblk, T, tblk, a->score_matrix, a->param.gap_open, a->param.gap_extend, a->param.x_dropoff, a->state_array, a->score_array, a->edit_script,
                    a->edit_start_offset, &a->edit_block, forward, qe, te);
        script_to_aligned_string(Q, T, qe, te, &a->edit_block, forward, tq, tt);
        ++F.blocks;
        const bool full_map = qblk - qe <= 20 || tblk - te <= 20;
        if (!full_map || last) {
            F.cols += (int64_t)tq.size();
            if (!full_map) F.xdrop_end = 1;
            if (last && (qblk < query_size - qidx || tblk < target_size - tidx)) F.sized_last = 1;
            break;
        }
        int qcnt = 0, tcnt = 0, acnt = 0;
        if (!trim_mismatch_end(tq.data(), tt.data(), (int)tq.size(), 4, qcnt, tcnt, acnt)) { F.failed_trim = 1; break; }
        F.cols += (int64_t)tq.size() - acnt;
        qidx += qe - qcnt;
        tidx += te - tcnt;
    }
    return F;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    FILE* sout = fopen(argv[3], "wb");
    if (!in || !out || !sout) return 2;
    const int64_t ref_size = rd(in), nreads = rd(in), ncand = rd(in);
    std::vector<char> ref((size_t)ref_size + 1, 0);
    if (fread(ref.data(), 1, (size_t)ref_size, in) != (size_t)ref_size) abort();
    std::vector<std::vector<char> > fwd((size_t)nreads), rev((size_t)nreads);
    for (int64_t i = 0; i < nreads; ++i) {
        const int64_t L = rd(in);
        fwd[i].assign((size_t)L + 1, 0);
        if (L && fread(fwd[i].data(), 1, (size_t)L, in) != (size_t)L) abort();
        rev[i] = fwd[i];
        std::reverse(rev[i].begin(), rev[i].begin() + L);
        for (int64_t j = 0; j < L; ++j) {
            char& c = rev[i][j];
            c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
        }
    }
    XdropAligner* aligner = new XdropAligner(0);
    TempResult* tr = create_temp_result();
    std::vector<char> qstr, tstr;
    AlignInfo alns[4];
    for (int64_t ci = 0; ci < ncand; ++ci) {
        const int64_t read = rd(in), chain = rd(in), loc1 = rd(in), loc2 = rd(in), score = rd(in);
        candidate_save can;
        memset(&can, 0, sizeof(can));
        can.loc1 = loc1; can.loc2 = loc2; can.score = (int)score; can.chain = chain ? 'R' : 'F';
        const int read_len = (int)fwd[read].size() - 1;
        int naln = 0, ntr = 0;
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        const bool ok = extend_candidate(can, aligner, ref.data(), ref_size, fwd[read].data(), rev[read].data(), qstr, tstr, (int)read, read_len, alns, &naln, tr, ntr);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if ((ok ? 1 : 0) != ntr || naln != ntr) abort();
        const int64_t cols = aligner->aln_size, lraw = (int64_t)aligner->left_qaln.size(), rraw = (int64_t)aligner->right_qaln.size();
        if (cols != std::max<int64_t>(lraw - 1, 0) + rraw) abort();
        std::vector<char> qmap(aligner->qaln, aligner->qaln + cols), smap(aligner->taln, aligner->taln + cols);
        const int64_t qb = aligner->qoff, qe = aligner->qend, ts = aligner->toff, te = aligner->tend;
        if (ok != (qe - qb >= 1000)) abort();
        if (ok && (tr->qb != qb || tr->qe != qe || tr->qs != read_len || strlen(tr->qmap) != (size_t)cols || memcmp(tr->qmap, qmap.data(), (size_t)cols) ||
                   memcmp(tr->smap, smap.data(), (size_t)cols) || alns[0].soff != tr->sb || alns[0].send != tr->se || alns[0].qdir != can.chain))
            abort();
        int64_t matches = 0;
        for (int64_t k = 0; k < cols; ++k) matches += qmap[k] == smap[k];
        // the start point inside the window is left_ref_size: extract_sequences' arithmetic again
        const long ref_start = (long)loc1 - 1;
        const int read_start = (int)loc2;
        const long L = std::min<long>(read_start, ref_start);
        const long left = std::min(ref_start, (long)(L * 1.2));
        const DirFacts Lf = probe(aligner, qstr.data() + read_start - 1, read_start, tstr.data() + left - 1, (int)left, false);
        const DirFacts Rf = probe(aligner, qstr.data() + read_start, read_len - read_start, tstr.data() + left, (int)tstr.size() - (int)left, true);
        if (Lf.cols != lraw || Rf.cols != rraw) { fprintf(stderr, "candidate %lld: the probe disagrees with go\n", (long long)ci); return 3; }
        const int64_t ns = (int64_t)(t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec);
        const int64_t rec[21] = {ok, qb, qe, read_len, ts, te, cols, lraw, rraw, ok ? tr->sb : 0, ok ? tr->se : 0, matches,
                                 Lf.blocks, Lf.sized_last, Lf.xdrop_end, Lf.failed_trim, Rf.blocks, Rf.sized_last, Rf.xdrop_end, Rf.failed_trim, ns};
        fwrite(rec, sizeof(rec), 1, out);
        fwrite(&cols, sizeof(cols), 1, sout);
        fwrite(qmap.data(), 1, (size_t)cols, sout);
        fwrite(smap.data(), 1, (size_t)cols, sout);
    }
    fclose(out);
    fclose(sout);
    return 0;
}
