// cns_table.hip — mecat2cns' consensus table, tallied on the device from the aligned strings of the accepted alignments
// (reference: meap_add_one_aln, mecat2cns/mecat_correction.cpp:36-60, called for every accepted alignment at :439 / :502 with the
// gap-normalised strings and m5soff; CnsTableItem {base, mat_cnt, ins_cnt, del_cnt}, reads_correction_aux.h:11-19; and the per-position
// classification identify_one_consensus_item, mecat_correction.cpp:14-24, FMAT 1 / FDEL 2 / FINS 4 / UNDS 8, :9-12).
//
// The reference walks one alignment column by column with a running template position.  Restated for a parallel walk: the template
// position of column i is p(i) = soff + the number of columns before i whose template character is not '-', and
//     both characters '-'                nothing
//     both bases (equal: O(ND) output)   ++mat_cnt[p(i)]
//     query '-', template base           ++ins_cnt[p(i)]
//     template '-'                       the maximal run of columns with template '-' adds ONE ++del_cnt[p - 1] if any of its columns has
//                                        a query base (the reference counts at the first such column and jumps to the end of the run;
//                                        double-gap columns in front of it are stepped over one by one, later ones are swallowed)
// A mismatch column does not occur in these strings (the reference asserts on one); here it would count as a match.
//
//   cns_table_tally    one WAVE per accepted alignment, 64 columns per step: two ballots give the gap masks of the step, a popcount of
//                      the template-base mask below a lane gives p(i); the template position so far and "the s-gap run that reaches the
//                      end of the step has been counted" are carried from step to step (both wave-uniform).  Every lane does at most
//                      one no-return 32-bit atomic add (1 << 8, 1 << 16 or 1 << 24, agent scope): a template takes at most 60 / 100
//                      alignments (255 through the test hook), so no byte carries into the next one and the sums do not depend on the
//                      order of arrival.  Consecutive template-base lanes hit consecutive words.  p - 1 == -1 (a run in front of the
//                      first template base at soff == 0; the reference would write below its array) and anything outside the template's
//                      table is dropped.
//   cns_table_finish   one LANE per table word, behind the tally on the same stream: base = the template's own letter where mat_cnt > 0
//                      (every match column of every alignment would write that letter: the reference's last-writer value), else 'N'; the
//                      ident byte in double arithmetic as the reference writes it.  The word is stored whole.
#include <algorithm>
#include <vector>

#include "common.h"
#include "cns_table.h"

namespace {

__global__ __launch_bounds__(256) void cns_table_tally(const char* __restrict__ str, const CnsTabItem* __restrict__ items, int n_items, uint32_t* __restrict__ table) {
    const int lane = lane_id();
    const unsigned long long lt = (1ull << lane) - 1ull;                // the lanes below this one
    for (size_t a = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); a < (size_t)n_items; a += (size_t)gridDim.x * 4) {
        const CnsTabItem it = items[a];
        const char* __restrict__ q = str + it.off;
        const char* __restrict__ s = q + it.aln_size + 1;
        uint32_t* __restrict__ tab = table + it.tab;
        const int n = it.aln_size;
        int pos = it.soff;                      // template position of the step's first column
        bool counted = false;                   // the s-gap run that reached the end of the previous step has added its del
        char nq = 0, ns = 0;
        if (lane < n) { nq = q[lane]; ns = s[lane]; }
        for (int c0 = 0; c0 < n; c0 += 64) {
            const bool valid = c0 + lane < n;
            const char cq = nq, cs = ns;
            if (c0 + 64 + lane < n) { nq = q[c0 + 64 + lane]; ns = s[c0 + 64 + lane]; }      // the next step's characters, in flight under this step
            const unsigned long long sg = __ballot(valid && cs == '-');
            const unsigned long long qg = __ballot(valid && cq == '-');
            const unsigned long long sb = __ballot(valid && cs != '-');      // columns with a template base
            const unsigned long long qb = sg & ~qg;                             // template gap under a query base
            const int p = pos + __popcll(sb & lt);
            int idx = -1;
            uint32_t add = 0;
            if ((sb >> lane) & 1ull) {
                idx = p;
                add = ((qg >> lane) & 1ull) ? (1u << 16) : (1u << 8);
            } else if ((qb >> lane) & 1ull) {
                // this lane's run starts behind the highest column below it that is no template gap, or comes in from the previous step
                const unsigned long long below = ~sg & lt;
                const int a0 = below ? 64 - __clzll((long long)below) : 0;
                const unsigned long long run = lt & ~((1ull << a0) - 1ull);      // the run's columns in front of this lane (a0 <= lane)
                if ((qb & run) == 0 && !(below == 0 && counted)) { idx = p - 1; add = 1u << 24; }
            }
            if (idx >= 0 && idx < it.tab_len) (void)__hip_atomic_fetch_add(tab + idx, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pos += __popcll(sb);
            if (sg >> 63) {                     // the step ends inside a run
                const unsigned long long z = ~sg;
                const int a63 = z ? 64 - __clzll((long long)z) : 0;              // (<= 63: bit 63 of z is clear)
                counted = (qb & (~0ull << a63)) != 0 || (z == 0 && counted);
            } else counted = false;
        }
    }
}

__global__ __launch_bounds__(256) void cns_table_finish(uint32_t* __restrict__ table, uint8_t* __restrict__ ident, long long n_words, const uint32_t* __restrict__ pac,
                                                        const long long* __restrict__ first, const int32_t* __restrict__ voloff, int n_tmpl,
                                                        const char* __restrict__ letters) {
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (long long)gridDim.x * 256) {
        const uint32_t x = table[w];
        const int mat = (int)((x >> 8) & 255u), ins = (int)((x >> 16) & 255u), del = (int)(x >> 24);
        uint32_t base = 'N';
        if (mat > 0) {
            if (letters) base = (uint8_t)letters[w];
            else {
                int lo = 0, hi = n_tmpl;          // first[lo] <= w < first[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (first[mid] <= w) lo = mid; else hi = mid;
                }
                base = (0x54474341u >> (pac_base(pac, (int64_t)voloff[lo] + (int64_t)(w - first[lo])) << 3)) & 0xffu;      // "ACGT"
            }
        }
        const int cov = mat + ins;              // identify_one_consensus_item, mecat_correction.cpp:14-24
        uint32_t id = 0;
        if ((double)mat >= (double)cov * 0.8) id |= 1u;      // FMAT
        if ((double)ins >= (double)cov * 0.8) id |= 4u;      // FINS
        if (!id) id |= 8u;                                   // UNDS
        if ((double)del >= (double)cov * 0.4) id |= 2u;      // FDEL
        table[w] = (x & 0xffffff00u) | base;
        ident[w] = (uint8_t)id;
    }
}

}  // namespace

int cns_table_launch(mhip_ctx* c, const mhip_volume* vol, const char* d_str, const CnsTabItem* d_items, int n_items, uint32_t* d_table, uint8_t* d_ident,
                     long long n_words, const long long* d_first, const int32_t* d_voloff, int n_tmpl, const char* d_letters) {
    if (n_words <= 0) return 0;
    if (n_words > (long long)0x7fffffff * 256) { mhip_set_error("cns table: too many table positions in one launch"); return -1; }
    HIPCHK(hipMemsetAsync(d_table, 0, sizeof(uint32_t) * (size_t)n_words, c->stream));
    if (n_items > 0)
        LAUNCH(c, "cns_table_tally", cns_table_tally, (unsigned)std::min<size_t>(((size_t)n_items + 3) / 4, (size_t)c->num_cus * 64), 256, 0, d_str, d_items, n_items, d_table);
    LAUNCH(c, "cns_table_finish", cns_table_finish, (unsigned)((n_words + 255) / 256), 256, 0, d_table, d_ident, n_words, (const uint32_t*)(vol ? vol->d_pac : nullptr),
           d_first, d_voloff, n_tmpl, d_letters);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" {

// TEST HOOK (tests/test_gpu_cns_table.py): the two kernels above over `n_pairs` pairs of host strings in mhip_debug_push_gaps' layout
// (pair p: q at buf + off[p], its partner at q + len[p] + 1), all of them alignments to ONE template of tmpl_len letters, pair p starting
// at template position soff[p].  -> table_out[tmpl_len] ({base, mat, ins, del} bytes), ident_out[tmpl_len].  Refused before anything is
// launched: more than 255 pairs (a count byte would carry), a mismatch column, a pair whose template span leaves [0, tmpl_len).
int mhip_debug_cns_table(mhip_ctx* c, const char* buf, int64_t bytes, const int64_t* off, const int32_t* len, const int32_t* soff, int n_pairs,
                         const char* tmpl_letters, int tmpl_len, mhip_cns_table_item* table_out, uint8_t* ident_out) {
    HIPCHK(hipSetDevice(c->device));
    if (n_pairs < 0 || n_pairs > 255) { mhip_set_error("cns table: %d pairs (at most 255: the counts are bytes)", n_pairs); return -1; }
    if (tmpl_len <= 0) { mhip_set_error("cns table: empty template"); return -1; }
    std::vector<CnsTabItem> items((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        if (off[p] < 0 || len[p] < 0 || off[p] + 2 * ((int64_t)len[p] + 1) > bytes) { mhip_set_error("cns table: pair %d lies outside the buffer", p); return -1; }
        const char* q = buf + off[p];
        const char* s = q + len[p] + 1;
        int64_t span = 0;
        for (int i = 0; i < len[p]; ++i) {
            if (q[i] != '-' && s[i] != '-' && q[i] != s[i]) { mhip_set_error("cns table: pair %d has a mismatch column (%d)", p, i); return -1; }
            span += s[i] != '-';
        }
        if (soff[p] < 0 || (int64_t)soff[p] + span > tmpl_len) { mhip_set_error("cns table: pair %d leaves the template", p); return -1; }
        CnsTabItem& it = items[(size_t)p];
        it.off = (unsigned long long)off[p]; it.tab = 0; it.aln_size = len[p]; it.soff = soff[p]; it.tab_len = tmpl_len; it.pad = 0;
    }
    char *d_buf, *d_let;
    CnsTabItem* d_items;
    uint32_t* d_tab;
    uint8_t* d_id;
    if (c->scratch("ct_buf", (size_t)std::max<int64_t>(bytes, 1), (void**)&d_buf)) return -1;
    if (c->scratch("ct_items", sizeof(CnsTabItem) * (size_t)std::max(n_pairs, 1), (void**)&d_items)) return -1;
    if (c->scratch("ct_let", (size_t)tmpl_len, (void**)&d_let)) return -1;
    if (c->scratch("ct_tab", sizeof(uint32_t) * (size_t)tmpl_len, (void**)&d_tab)) return -1;
    if (c->scratch("ct_id", (size_t)tmpl_len, (void**)&d_id)) return -1;
    if (bytes > 0) HIPCHK(hipMemcpyAsync(d_buf, buf, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    if (n_pairs > 0) HIPCHK(hipMemcpyAsync(d_items, items.data(), sizeof(CnsTabItem) * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_let, tmpl_letters, (size_t)tmpl_len, hipMemcpyHostToDevice, c->stream));
    if (cns_table_launch(c, nullptr, d_buf, d_items, n_pairs, d_tab, d_id, tmpl_len, nullptr, nullptr, 0, d_let)) return -1;
    HIPCHK(hipMemcpyAsync(table_out, d_tab, sizeof(uint32_t) * (size_t)tmpl_len, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ident_out, d_id, (size_t)tmpl_len, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));      // (`items` lives until here)
    return 0;
}

}  // extern "C"
