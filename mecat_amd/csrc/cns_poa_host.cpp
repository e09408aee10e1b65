// cns_poa_host.cpp — cns_poa.h for the host, behind a C entry point over one packed case (libcns_poa_host.so: plain g++, no HIP).  The
// tests pin this build to the compiled reference and then use it as the expected value of the device's.  With -DCNS_POA_MAIN the same
// file is a stand-alone program that runs a packed fixture (tests/cns_poa_cases.py: write_cases) through the header and compares with
// the strings recorded in it — the program to build with a sanitizer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "cns_poa.h"
#include "cns_reads.h"
#include "cns_text.h"

namespace {

struct HostPieces {
    const char* buf;
    const int64_t* off;
    const int32_t* len;
    const int32_t* pc;      // this window's records: aln, col, ncols, sb_out
    void operator()(int k, const char** q, const char** t, int* ncols, int* sb_out) const {
        const int32_t* r = pc + 4 * (size_t)k;
        *q = buf + off[r[0]] + r[1];
        *t = *q + len[r[0]] + 1;
        *ncols = r[2];
        *sb_out = r[3];
    }
};

}  // namespace

extern "C" {

enum { CNS_POA_INFO = 14 };      // per window: return code, the bound's nodes and edges, CnsPoaStats

int cns_poa_host_info_words(void) { return CNS_POA_INFO; }
int cns_poa_host_stats_bytes(void) { return (int)sizeof(CnsPoaStats); }
int64_t cns_poa_host_words(int64_t nodes, int64_t edges) { return cns_poa_words(nodes, edges); }
int cns_poa_host_min_weight(int cov) { return cns_poa_min_weight(cov); }

// the corrected reads' record rule (cns_reads.h), the code cns_reads_records runs: records of a target of `size` letters, and block k of
// a segment [beg, end) as out[4] = L, R, range_beg, range_end
int64_t cns_reads_host_blocks(int64_t size) { return cns_reads_blocks(size); }
void cns_reads_host_block(int64_t size, int64_t k, int64_t beg, int64_t end, int64_t* out) {
    long long L, R, rb, re;
    cns_reads_block(size, k, beg, end, &L, &R, &rb, &re);
    out[0] = L; out[1] = R; out[2] = rb; out[3] = re;
}

// the corrected reads' text rule (cns_text.h), the code cns_text_write runs: characters of a record's header line and of the whole record,
// and character l of the header line (0 behind its newline)
int cns_text_host_header_len(int32_t read_id, int32_t range_beg, int32_t range_end, int32_t size) { return cns_text_header_len(read_id, range_beg, range_end, size); }
int64_t cns_text_host_record_len(int32_t read_id, int32_t range_beg, int32_t range_end, int32_t size) { return cns_text_record_len(read_id, range_beg, range_end, size); }
int cns_text_host_header_char(int32_t read_id, int32_t range_beg, int32_t range_end, int32_t size, int l) { return cns_text_header_char(read_id, range_beg, range_end, size, l); }

// One template: n_alns alignments (alignment a: qaln at buf + off[a], len[a] characters + NUL, saln right behind it), n_windows windows
// as triples (sb, se, cov), their pieces as records (aln, col, ncols, sb_out), window w owning [piece_begin[w], piece_begin[w + 1]).
// -> out: the windows' consensus strings one behind the other, out_begin[n_windows + 1]; info[CNS_POA_INFO * w ..] may be NULL.
// Returns 0; -1 for a record that leaves its alignment or a window that is not sb < se; -2 when out_cap is too small; 100 + code when
// the routine returned a CNS_POA_E* code (a bug: the workspace is sized by the header's own bound).
int cns_poa_host_case(const char* buf, const int64_t* off, const int32_t* len, int n_alns, const int32_t* windows, int n_windows, const int32_t* pieces,
                      const int64_t* piece_begin, char* out, int64_t out_cap, int64_t* out_begin, int32_t* info) {
    std::vector<int32_t> ws;
    std::vector<char> cns;
    int64_t used = 0;
    out_begin[0] = 0;
    for (int w = 0; w < n_windows; ++w) {
        const int32_t sb = windows[3 * w], se = windows[3 * w + 1], cov = windows[3 * w + 2];
        if (sb >= se || piece_begin[w] > piece_begin[w + 1] || (int64_t)se - sb > 0x3fffffff) return -1;
        const int np = (int)(piece_begin[w + 1] - piece_begin[w]);
        HostPieces get = {buf, off, len, pieces + 4 * piece_begin[w]};
        long long ins = 0, calls = 0;
        for (int k = 0; k < np; ++k) {
            const int32_t* r = get.pc + 4 * (size_t)k;
            if (r[0] < 0 || r[0] >= n_alns || r[1] < 0 || r[2] < 1 || (int64_t)r[1] + r[2] > len[r[0]]) return -1;
            const char *q, *t;
            int ncols, sb_out;
            get(k, &q, &t, &ncols, &sb_out);
            long long sum = 0;
            cns_poa_count(q, t, ncols, &sum, &calls);
            ins += sum;
            assert(sum <= ncols);
        }
        const long long blen = (long long)se - sb + 1;
        const long long nodes = blen + 2 + ins, edges = blen + 1 + calls;
        if (nodes > 0x3fffffff || edges > 0x3fffffff) return -1;
        ws.resize((size_t)cns_poa_words(nodes, edges));
        cns.resize((size_t)nodes);
        int32_t n = 0;
        CnsPoaStats st;
        const int rc = cns_poa_window(sb, se, cov, get, np, ws.data(), (int32_t)nodes, (int32_t)edges, cns.data(), (int32_t)(nodes - 2), &n, &st);
        // the bound of the header's CAPACITIES comment
        assert(rc != CNS_POA_OK || (st.nodes <= nodes && st.edges <= edges && st.queue <= nodes && st.frames <= nodes && st.members <= nodes && n <= nodes - 2));
        if (info) {
            int32_t* o = info + (size_t)CNS_POA_INFO * w;
            o[0] = rc; o[1] = (int32_t)nodes; o[2] = (int32_t)edges;
            memcpy(o + 3, &st, sizeof(st));
        }
        if (rc) return 100 + rc;
        if (used + n > out_cap) return -2;
        memcpy(out + used, cns.data(), (size_t)n);
        used += n;
        out_begin[w + 1] = used;
    }
    return 0;
}

}  // extern "C"

static_assert(sizeof(CnsPoaStats) == 4 * (CNS_POA_INFO - 3), "info layout");

#ifdef CNS_POA_MAIN
// the packed fixture: int32 words and raw bytes, see tests/cns_poa_cases.py write_cases
namespace {
struct Reader {
    FILE* f;
    int32_t i32() { int32_t v = 0; if (fread(&v, 4, 1, f) != 1) { fprintf(stderr, "short file\n"); exit(2); } return v; }
    void bytes(char* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short file\n"); exit(2); } }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    Reader r = {fopen(argv[1], "rb")};
    if (!r.f) { perror(argv[1]); return 2; }
    if (r.i32() != 0x504f4131) { fprintf(stderr, "not a case file\n"); return 2; }
    const int ncases = r.i32();
    if (!r.i32()) { fprintf(stderr, "the file holds no pieces and strings\n"); return 2; }
    long long nwin_all = 0, differ = 0;
    for (int c = 0; c < ncases; ++c) {
        r.i32();      // (fresh cursors per window: the pieces in the file already are what that gives)
        const int na = r.i32();
        std::vector<int64_t> off((size_t)na);
        std::vector<int32_t> len((size_t)na);
        std::string buf;
        for (int a = 0; a < na; ++a) {
            r.i32(); r.i32();
            len[(size_t)a] = r.i32();
            off[(size_t)a] = (int64_t)buf.size();
            const size_t n = (size_t)len[(size_t)a];
            buf.resize(buf.size() + 2 * (n + 1), '\0');
            r.bytes(&buf[(size_t)off[(size_t)a]], n);
            r.bytes(&buf[(size_t)off[(size_t)a] + n + 1], n);
        }
        const int nw = r.i32();
        std::vector<int32_t> win(3 * (size_t)nw);
        for (auto& v : win) v = r.i32();
        std::vector<int64_t> pb((size_t)nw + 1);
        for (auto& v : pb) v = r.i32();
        std::vector<int32_t> pc(4 * (size_t)pb[(size_t)nw]);
        for (auto& v : pc) v = r.i32();
        std::string want;
        std::vector<int64_t> wb((size_t)nw + 1, 0);
        for (int w = 0; w < nw; ++w) {
            const int n = r.i32();
            want.resize(want.size() + (size_t)n);
            r.bytes(&want[(size_t)wb[(size_t)w]], (size_t)n);
            wb[(size_t)w + 1] = (int64_t)want.size();
        }
        std::string got(want.size() + 1024, '\0');
        std::vector<int64_t> gb((size_t)nw + 1, 0);
        const int rc = cns_poa_host_case(buf.data(), off.data(), len.data(), na, win.data(), nw, pc.data(), pb.data(), &got[0], (int64_t)got.size(), gb.data(), nullptr);
        if (rc) { printf("case %d: return code %d\n", c, rc); ++differ; continue; }
        for (int w = 0; w < nw; ++w)
            differ += gb[(size_t)w + 1] - gb[(size_t)w] != wb[(size_t)w + 1] - wb[(size_t)w] ||
                      memcmp(&got[(size_t)gb[(size_t)w]], &want[(size_t)wb[(size_t)w]], (size_t)(wb[(size_t)w + 1] - wb[(size_t)w])) != 0;
        nwin_all += nw;
    }
    printf("cns_poa: %d cases, %lld windows, %lld differ from the recorded strings\n", ncases, nwin_all, differ);
    return differ != 0;
}
#endif
