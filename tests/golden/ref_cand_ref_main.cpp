// Recorder linked into the UNMODIFIED mecat2ref by tests/golden/make_golden_ref_cand.py (build container only; nothing compiled from it
// is committed).  The generator compiles the reference's mecat2ref and common sources where they lie into a temporary directory, makes
// `extend_candidate` and `rescue_clipped_align` weak in the object of mecat2ref_aux.cpp and links this file, whose definitions then take
// their place:
//   extend_candidate      stores its candidate_save argument and returns false, so no read ever gets an alignment: every read ends round 1
//                         with naln == 0 and round 2 (2 000-base segments, stride 5) runs for every read too
//   rescue_clipped_align  is called once per read and round behind the extend_candidate loop, with the round's segment length as
//                         block_size: the end-of-list marker (with naln == 0 the original does nothing)
// Records are 12 int64 each, appended to the file named by REF_CAND_OUT:
//   {1, read, loc1, loc2, left1, left2, right1, right2, score, num1, num2, chain ('F' -> 0, 'R' -> 1)}
//   {2, read, block_size, 0 ...}
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mecat2ref_aux.h"

static FILE* rec_file() {
    static FILE* f = NULL;
    if (!f) {
        const char* p = getenv("REF_CAND_OUT");
        f = fopen(p ? p : "ref_cand.bin", "wb");
        if (!f) abort();
    }
    return f;
}

bool extend_candidate(candidate_save& can, GapAligner*, const char*, const long, const char*, const char*, std::vector<char>&, std::vector<char>&,
                      int read_name, int, AlignInfo*, int*, TempResult*, int&) {
    const int64_t r[12] = {1, read_name, can.loc1, can.loc2, can.left1, can.left2, can.right1, can.right2, can.score, can.num1, can.num2, can.chain == 'R'};
    fwrite(r, sizeof(r), 1, rec_file());
    return false;
}

void rescue_clipped_align(AlignInfo*, int&, TempResult*, int&, GapAligner*, const char*, const long, const char*, const char*, std::vector<char>&,
                          std::vector<char>&, int read_name, int, int block_size, int, Back_List*, Back_List*, double) {
    const int64_t r[12] = {2, read_name, block_size, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    fwrite(r, sizeof(r), 1, rec_file());
    fflush(rec_file());
}
