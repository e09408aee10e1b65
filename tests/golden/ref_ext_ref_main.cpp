// Recorder for tests/golden/make_golden_ref_ext.py (build container only; nothing compiled from it is committed).  The generator compiles
// the reference's mecat2ref_aux.cpp, output.cpp and common sources where they lie into a temporary directory and links this main with
// them: it calls the UNMODIFIED extend_candidate (mecat2ref/mecat2ref_aux.cpp:123-183) with a DiffAligner(0), as reference_mapping does
// (mecat2ref_impl_large.cpp:328-332, :566-582), once per given candidate, and records what the aligner holds afterwards.
//
// Input (argv[1]), int64 little-endian: ref_size, nreads, ncand; the reference's letters as the tool holds them (one behind the other,
// upper-cased); per read its length and letters; per candidate {read, chain (0 'F' / 1 'R'), loc1, loc2, score}.
// The reverse strand is made the way reference_mapping makes it (:374-408): the read reversed, upper-case A, C, G, T complemented.
// Output argv[2]: per candidate 20 int64
//   {ok, qb, qe, qs, ts, te, cols, lcols, rcols, sb, se,  L: blocks, sized_last, fallback, tail_rows,  R: the same four,  ns}
//   ts / te = the aligner's target_start / target_end inside the window; sb / se = the TempResult's (ok results only);
//   ns = nanoseconds of the extend_candidate call.
// The per-direction facts come from a second pass over the same sequences that chains the reference's own retrieve_next_aln_block, Align
// and trim_mismatch_end the way dw_in_one_direction does (diff_gapalign.cpp:221-292) and must arrive at the same number of columns:
//   blocks      blocks aligned;  sized_last = the last block was cut by the `x 1.2` rule (gapalign.cpp:26-29), not by what was left
//   fallback    kept blocks whose Align reached neither end (the best point, diff_gapalign.cpp:197-207)
//   tail_rows   the most indel columns any block's trim_mismatch_end walked back over
// Output argv[3]: per candidate int64 cols, then the query string and the target string (cols bytes each).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <vector>

#include "../common/diff_gapalign.h"
#include "../common/gapalign.h"
#include "mecat2ref_aux.h"
#include "output.h"

int Align(const char* query, const int q_len, const char* target, const int t_len, const int band_tolerance, const int get_aln_str, Alignment* align,
          int* V, int* U, DPathData2* d_path, PathPoint* aln_path, const int right_extend);

static int64_t rd(FILE* f) {
    int64_t v;
    if (fread(&v, sizeof(v), 1, f) != 1) abort();
    return v;
}

struct DirFacts { int64_t blocks, sized_last, fallback, tail_rows, cols; };

static DirFacts probe(DiffAligner* a, const char* query, const int query_size, const char* target, const int target_size, const int right) {
    DirFacts F = {0, 0, 0, 0, 0};
    int qidx = 0, tidx = 0, qblk, tblk;
    const char *s1, *s2;
    while (1) {
        std::fill(a->dynq, a->dynq + a->param.row_size, 0);
        std::fill(a->dynt, a->dynt + a->param.column_size, 0);
        const bool last = retrieve_next_aln_block(query, qidx, query_size, target, tidx, target_size, a->param.segment_size, right, s1, s2, qblk, tblk);
        const int reached = Align(s1, qblk, s2, tblk, 0.3 * std::max(qblk, tblk), 400, a->align, a->dynq, a->dynt, a->d_path, a->aln_path, right);
        ++F.blocks;
        int qcnt = 0, tcnt = 0, acnt = 0;
        if (!trim_mismatch_end(a->align->q_aln_str, a->align->t_aln_str, a->align->aln_str_size, 4, qcnt, tcnt, acnt)) break;
        if (last && (qblk < query_size - qidx || tblk < target_size - tidx)) F.sized_last = 1;
        if (!reached) ++F.fallback;
        int64_t rows = 0;
        for (int k = a->align->aln_str_size - acnt; k < a->align->aln_str_size; ++k)
            if (a->align->q_aln_str[k] != a->align->t_aln_str[k]) ++rows;
        F.tail_rows = std::max(F.tail_rows, rows);
        const bool full_map = qblk - a->align->aln_q_e <= 20 || tblk - a->align->aln_t_e <= 20;
        if (last || !full_map) { qcnt -= 4; tcnt -= 4; acnt -= 4; }
        F.cols += a->align->aln_str_size - acnt;
        if (last || !full_map) break;
        qidx += a->align->aln_q_e - qcnt;
        tidx += a->align->aln_t_e - tcnt;
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
    DiffAligner* aligner = new DiffAligner(0);
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
        OutputStore* rs = aligner->result;
        const int64_t cols = rs->out_store_size, lcols = rs->left_store_size, rcols = rs->right_store_size;
        std::vector<char> qmap(rs->out_store1, rs->out_store1 + cols), smap(rs->out_store2, rs->out_store2 + cols);
        const int64_t qb = rs->query_start, qe = rs->query_end, ts = rs->target_start, te = rs->target_end;
        if (ok && (tr->qb != qb || tr->qe != qe || tr->qs != read_len || strlen(tr->qmap) != (size_t)cols || memcmp(tr->qmap, qmap.data(), (size_t)cols) ||
                   memcmp(tr->smap, smap.data(), (size_t)cols) || alns[0].soff != tr->sb || alns[0].send != tr->se || alns[0].qdir != can.chain))
            abort();
        // the start point inside the window: target_start + the target bases of the left part
        int64_t tstart = ts;
        for (int64_t k = 0; k < lcols; ++k)
            if (smap[k] != '-') ++tstart;
        const int read_start = (int)loc2;
        const DirFacts L = probe(aligner, qstr.data() + read_start - 1, read_start, tstr.data() + tstart - 1, (int)tstart, 0);
        const DirFacts R = probe(aligner, qstr.data() + read_start, read_len - read_start, tstr.data() + tstart, (int)tstr.size() - (int)tstart, 1);
        if (L.cols != lcols || R.cols != rcols) { fprintf(stderr, "candidate %lld: the probe disagrees with go\n", (long long)ci); return 3; }
        const int64_t ns = (int64_t)(t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec);
        const int64_t rec[20] = {ok, qb, qe, read_len, ts, te, cols, lcols, rcols, ok ? tr->sb : 0, ok ? tr->se : 0,
                                 L.blocks, L.sized_last, L.fallback, L.tail_rows, R.blocks, R.sized_last, R.fallback, R.tail_rows, ns};
        fwrite(rec, sizeof(rec), 1, out);
        fwrite(&cols, sizeof(cols), 1, sout);
        fwrite(qmap.data(), 1, (size_t)cols, sout);
        fwrite(smap.data(), 1, (size_t)cols, sout);
    }
    fclose(out);
    fclose(sout);
    return 0;
}
