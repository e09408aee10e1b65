// cns_accept.hip — mecat2cns' candidate accept loop on top of the device re-aligner.
//
// Replaces, for a batch of template reads, the front half of consensus_one_read_can_pacbio / consensus_one_read_can_nanopore
// (mecat2cns/mecat_correction.cpp:388-450, 452-515): everything up to the point where an accepted alignment is handed to the
// consensus table (meap_add_one_aln) and to CnsAlns::add_aln.  The reference walks a template's candidates one by one —
//     sort by (score desc, qid, qext)                                             :362-370, :409
//     for each, while fewer than 60 (PacBio) / 100 (nanopore) are accepted and fewer than 200 were looked at:
//         skip a query read that was already accepted (std::set used_ids)         :424
//         GetAlignment(error_rate 0.15 / 0.20, min_align_size)                    :431 (dw.cpp:482-553)
//         check_ovlp_mapping_range with min_mapping_ratio - 0.02                  :191-200, :432
//         check_cov_stats: the aligned template range must have >= 200 positions below coverage 20, then ++coverage   :372-386
//         normalize_gaps(qaln, saln, push = true) -> meap_add_one_aln, add_aln    reads_correction_aux.cpp:3-81
// — and every alignment depends on nothing but the two reads, so the <= 200 candidates of every template of the batch are
// re-aligned speculatively on the device (mhip_cns_align_candidates_dev, a slice of the batch's templates per launch), the sequential
// accept decisions are replayed over the results on host threads, and the gap-normalised strings of the ACCEPTED alignments are
// built on the device as well (cns_strings.hip) and copied into the result buffer while the next slice re-aligns.
// mhip_cns_accept_templates_ex adds what the reference does with those strings first: the consensus table of every template
// (meap_add_one_aln, :36-60, at :439 / :502) and its per-position classification (identify_one_consensus_item, :14-24), tallied
// from the strings while they are still in device memory (cns_table.hip) — and, asked for the table alone, never copies the strings.
// mhip_cns_accept_templates_plan adds what the reference decides from the table alone: the effective ranges (get_effective_ranges,
// :118-153, in the replay: cns_ranges.h), and behind a slice's table kernels the segments (consensus_worker, :203-239) and the windows
// that go to the POA (meap_consensus_one_segment, :81-108) — cns_plan.hip.
// mhip_cns_accept_templates_pieces adds what the reference does with a listed window first: every accepted alignment's part of it
// (CnsAln::retrieve_aln_subseqs, reads_correction_aux.h:47-68, called by meap_cns_one_indel, :62-78), as descriptors, behind a slice's
// plan while its strings are still in device memory — cns_pieces.hip.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <set>
#include <thread>
#include <vector>

#include <functional>

#include "common.h"
#include "cns_strings.h"
#include "cns_pieces.h"
#include "cns_poa_dev.h"
#include "cns_plan.h"
#include "cns_ranges.h"
#include "cns_table.h"

namespace {

struct CmpByScore {      // CmpExtensionCandidateByScore, mecat_correction.cpp:362-370
    bool operator()(const mhip_ext_candidate& a, const mhip_ext_candidate& b) const {
        if (a.score != b.score) return a.score > b.score;
        if (a.qid != b.qid) return a.qid < b.qid;
        return a.qext < b.qext;
    }
};

template <typename F>
void parallel_for(int64_t n, int nthreads, F f) {
    nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(nthreads, n));
    std::atomic<int64_t> next{0};
    auto body = [&]() {
        for (;;) {
            const int64_t i = next.fetch_add(1);
            if (i >= n) return;
            f(i);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; ++t) th.emplace_back(body);
    body();
    for (auto& x : th) x.join();
}

}  // namespace

extern "C" {

// The strings of a batch are gigabytes (24 GB at config 2), and pages that are touched for the first time cost more than the copy that
// fills them.  So the library keeps ONE released string buffer and
// hands it out again when the next batch fits it (mecat2cns works through its partitions batch after batch): pages that are mapped
// already.  mhip_cns_free parks a buffer it knows instead of freeing it; a larger request replaces the parked one.
namespace {
std::mutex g_strbuf_mu;
char* g_strbuf_parked = nullptr;          // released, reusable
size_t g_strbuf_parked_cap = 0;
std::map<void*, size_t> g_strbuf_out;     // handed to a caller: address -> capacity
std::set<void*> g_strbuf_reg;             // page-locked (hipHostRegister): the copy engine fills them without a staging copy, asynchronously
void strbuf_free(void* p) {               // (g_strbuf_mu held or not: only the set is shared)
    if (!p) return;
    bool reg;
    { std::lock_guard<std::mutex> lk(g_strbuf_mu); reg = g_strbuf_reg.erase(p) != 0; }
    if (reg) (void)hipHostUnregister(p);
    free(p);
}
// cap bytes (a multiple of 2 MB), touched and page-locked; registered buffers are noted in g_strbuf_reg
void* locked_alloc(size_t cap, int num_threads) {
    void* p = nullptr;
    const size_t two_mb = (size_t)2 << 20;
    if (posix_memalign(&p, two_mb, cap) != 0) return nullptr;
    (void)madvise(p, cap, MADV_HUGEPAGE);
    // first touch on the host threads (huge pages: 8 GB in 30 ms on 32 threads), then page-locked — 70 ms for 8 GB of touched pages, against
    // 0.4 s untouched and 1.9 s for a hipHostMalloc of the size (tools/dev/probes/pin_probe.hip)
    parallel_for((int64_t)(cap / two_mb), num_threads, [&](int64_t pg) { ((volatile char*)p)[(size_t)pg * two_mb] = 0; });
    const bool reg = hipHostRegister(p, cap, hipHostRegisterDefault) == hipSuccess;
    if (!reg) (void)hipGetLastError();      // stays pageable: the copies still work, through the runtime's staging
    if (reg) { std::lock_guard<std::mutex> lk(g_strbuf_mu); g_strbuf_reg.insert(p); }
    return p;
}
char* strbuf_get(size_t bytes, int num_threads) {
    {
        std::lock_guard<std::mutex> lk(g_strbuf_mu);
        if (g_strbuf_parked && g_strbuf_parked_cap >= bytes) {
            char* p = g_strbuf_parked;
            g_strbuf_out[p] = g_strbuf_parked_cap;
            g_strbuf_parked = nullptr;
            g_strbuf_parked_cap = 0;
            return p;
        }
    }
    const size_t two_mb = (size_t)2 << 20, cap = (bytes + bytes / 16 + two_mb - 1) & ~(two_mb - 1);
    void* p = locked_alloc(cap, num_threads);
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(g_strbuf_mu);
    g_strbuf_out[p] = cap;
    return (char*)p;
}
// a result buffer that the copy engine fills (the tables of a batch: 5 bytes per template base): page-locked from 64 MB on, plain
// malloc below; never parked — mhip_cns_free unregisters and frees it
void* result_alloc(size_t bytes, int num_threads) {
    if (bytes < ((size_t)64 << 20)) return malloc(std::max<size_t>(bytes, 1));
    const size_t two_mb = (size_t)2 << 20;
    return locked_alloc((bytes + two_mb - 1) & ~(two_mb - 1), num_threads);
}
}  // namespace

void mhip_cns_free(void* p) {
    if (!p) return;
    void* to_free = p;
    {
        std::lock_guard<std::mutex> lk(g_strbuf_mu);
        auto it = g_strbuf_out.find(p);
        if (it != g_strbuf_out.end()) {
            const size_t cap = it->second;
            g_strbuf_out.erase(it);
            if (cap > g_strbuf_parked_cap) {      // park this one, free what was parked (the smaller of the two)
                to_free = g_strbuf_parked;
                g_strbuf_parked = (char*)p;
                g_strbuf_parked_cap = cap;
            }
        }
    }
    strbuf_free(to_free);      // (a plain malloc'ed buffer — the accepted records, small string buffers — is just freed)
}

// gives the parked string buffer (see above) back to the system; buffers still in a caller's hands are not touched
void mhip_cns_release_parked(void) {
    void* p;
    {
        std::lock_guard<std::mutex> lk(g_strbuf_mu);
        p = g_strbuf_parked;
        g_strbuf_parked = nullptr;
        g_strbuf_parked_cap = 0;
    }
    strbuf_free(p);
}

// what mhip_cns_accept_templates_plan adds to the call
struct PlanArgs {
    bool want = false;
    int min_cov = 0, min_size = 0;
    mhip_cns_segment** seg = nullptr; int64_t** seg_begin = nullptr; mhip_cns_window** win = nullptr; int64_t* n_win = nullptr;
    int32_t** er = nullptr; int64_t** er_begin = nullptr;
    bool want_pieces = false;      // mhip_cns_accept_templates_pieces: the windows' pieces as well
    mhip_cns_piece** pc = nullptr; int64_t** pc_begin = nullptr;
    bool want_poa = false;         // mhip_cns_accept_templates_poa: the windows' consensus strings as well
    char** cns = nullptr; int64_t** cns_begin = nullptr;
};

// the body of the entry points; want_tab: the outputs behind out_jobs are filled as well; plan.want: the outputs of `plan` too
static int cns_accept_body(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin,
                           int num_templates, int tech, int min_align_size, double min_mapping_ratio, int num_threads, const bool want_str, const bool want_tab,
                           mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings, int64_t* out_strings_bytes,
                           int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident, int64_t** out_table_begin, const PlanArgs& plan) {
    HIPCHK(hipSetDevice(c->device));
    const bool want_plan = plan.want, want_pieces = plan.want && plan.want_pieces, want_poa = plan.want && plan.want_poa, build_tab = want_tab || want_plan;      // the plan reads the table: built on the device either way, copied only when asked for
    const int min_run = want_plan ? cns_plan_min_run(plan.min_size) : 0;
    *out_accepted = nullptr; *out_count = 0; *out_strings = nullptr; *out_strings_bytes = 0;
    if (out_jobs) *out_jobs = 0;
    if (num_templates <= 0) return 0;
    const int max_ext = 200;                                         // mecat_correction.cpp:412
    const int max_added = tech == 0 ? 60 : 100;                      // :407 ; MAX_CNS_OVLPS, reads_correction_aux.h:32
    const double error_rate = tech == 0 ? 0.15 : 0.20;               // :431 / :494
    const double ratio = min_mapping_ratio - 0.02;                   // :406
    const int start_id = vol->start_read_id, nreads = vol->num_reads;
    num_threads = std::max(1, num_threads);
    // MECAT_CNS_TIMES=1: where the call's wall time went, on stderr
    const bool times = getenv("MECAT_CNS_TIMES") != nullptr;
    double tk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_last = now();
    auto lap = [&](int k) { const double t = now(); tk[k] += t - t_last; t_last = t; };

    // 1. order of the reference's walk
    std::atomic<int> bad{0};
    parallel_for(num_templates, num_threads, [&](int64_t t) {
        mhip_ext_candidate* b = cands + tmpl_begin[t];
        mhip_ext_candidate* e = cands + tmpl_begin[t + 1];
        // std::sort, not stable_sort: the reference sorts the same array (file order of the partition) with the same comparator and
        // the same libstdc++ introsort (mecat_correction.cpp:409 / :472), so records that tie on (score, qid, qext) come out in the
        // reference's order exactly when the input order is the reference's — which is what the caller hands over
        std::sort(b, e, CmpByScore());
        for (mhip_ext_candidate* p = b; p < e; ++p) {
            if (p->sdir != 0 || p->qid < start_id || p->qid >= start_id + nreads || p->sid < start_id || p->sid >= start_id + nreads ||
                p->sid != b->sid) {
                bad = 1;
                continue;
            }
            // the record's read lengths are the volume's: the replay indexes the coverage array and the reads with them (the
            // reference has a fixed MAX_SEQ_SIZE array there; a record that disagrees with the volume is refused, not trusted)
            if (p->qsize != vol->h_offs[(size_t)(p->qid - start_id)].size || p->ssize != vol->h_offs[(size_t)(p->sid - start_id)].size) bad = 2;
        }
    });
    if (bad.load() == 2) { mhip_set_error("cns accept: a candidate's qsize / ssize differs from the read lengths of the volume"); return -1; }
    if (bad.load()) { mhip_set_error("cns accept: a candidate is outside the volume, has sdir != 0 or sits in another template's range"); return -1; }

    // the tables: one word per base of every template that has candidates, template after template
    std::vector<int64_t> TB;
    if (build_tab) {
        TB.assign((size_t)num_templates + 1, 0);
        for (int t = 0; t < num_templates; ++t)
            TB[(size_t)t + 1] = TB[(size_t)t] + (tmpl_begin[t + 1] > tmpl_begin[t] ? (int64_t)vol->h_offs[(size_t)(cands[tmpl_begin[t]].sid - start_id)].size : 0);
    }
    const int64_t TW = want_tab ? TB[(size_t)num_templates] : 0;
    // host buffers of the table outputs (filled by the copy stream), and the host arrays behind the slices' item copies: a set's arrays
    // live until the copies that follow the kernels which read them have completed (declared in front of `cleanup`, which waits for them)
    struct TabOut {
        uint32_t* tab = nullptr; uint8_t* id = nullptr; int64_t* begin = nullptr;
        ~TabOut() { mhip_cns_free(tab); mhip_cns_free(id); free(begin); }
    } tab_out;
    std::vector<CnsStrItem> hold_items[2];
    std::vector<CnsTabItem> hold_titems[2];
    std::vector<long long> hold_first[2];
    std::vector<int32_t> hold_voloff[2];
    auto hand_over_tables = [&]() -> int {          // (after the last copy has landed)
        tab_out.begin = (int64_t*)malloc(sizeof(int64_t) * ((size_t)num_templates + 1));
        if (!tab_out.begin) { mhip_set_error("out of memory"); return -1; }
        memcpy(tab_out.begin, TB.data(), sizeof(int64_t) * ((size_t)num_templates + 1));
        *out_table = (mhip_cns_table_item*)tab_out.tab; *out_ident = tab_out.id; *out_table_begin = tab_out.begin;
        tab_out.tab = nullptr; tab_out.id = nullptr; tab_out.begin = nullptr;
        return 0;
    };
    // the plan: effective ranges from the replay, segments and windows slice by slice in buffers of their own (their sizes are known
    // slice by slice only), put together at the end; the records are final when they leave the device
    struct PlanPiece {
        void* seg = nullptr; void* win = nullptr; int64_t nseg = 0, nwin = 0; long long bad = 0;
        // the slice's pieces (cns_pieces.hip): pc_cap slots of which the first pb[nwin] are records, pb[nwin + 1] counted from the slice's first
        void* pc = nullptr; int64_t* pb = nullptr; int64_t pc_cap = 0; long long pc_bad = 0;
        // the slice's consensus strings (cns_poa.hip): cn_cap bytes of which the first cb[nwin] are strings, cb[nwin + 1] counted from the slice's first
        void* cn = nullptr; int64_t* cb = nullptr; int64_t cn_cap = 0; long long cn_bad = 0;
    };
    // (bad: CnsPlanDev::d_bad, copied with the windows and looked at in hand_over_plan only, after every slice has run: the plan is refused
    // there; an overflow of the segment slots is refused by cns_plan_launch at once)
    struct PlanOut {
        std::vector<PlanPiece> pieces;
        ~PlanOut() { for (PlanPiece& p : pieces) { mhip_cns_free(p.seg); mhip_cns_free(p.win); mhip_cns_free(p.pc); mhip_cns_free(p.pb); mhip_cns_free(p.cn); mhip_cns_free(p.cb); } }
    } plan_out;
    std::vector<int64_t> SB, ERB;                 // per template: first segment; effective ranges (counts until the hand-over)
    std::vector<int32_t> ER;
    int64_t seg_total = 0, win_total = 0;
    long long poa_large = 0, poa_chunks = 0;      // windows that went to cns_poa_large, and its launches
    if (want_plan) { SB.assign((size_t)num_templates + 1, 0); ERB.assign((size_t)num_templates + 1, 0); }
    // the windows' pieces: every slice's records behind one another, piece_begin moved from slice-local to batch-wide numbers
    auto hand_over_pieces = [&](void** out_pc, int64_t** out_pb) -> int {
        int64_t total = 0;
        for (const PlanPiece& p : plan_out.pieces) {
            if (p.pc_bad) { mhip_set_error("cns pieces: an index left its array, or the pieces written are not the pieces counted"); return -1; }
            if (!p.pb) continue;
            const int64_t np = p.pb[p.nwin];
            if (p.pb[0] != 0 || np < 0 || np > p.pc_cap) { mhip_set_error("cns pieces: inconsistent counts (%lld pieces in %lld slots)", (long long)np, (long long)p.pc_cap); return -1; }
            total += np;
        }
        int64_t* pb = (int64_t*)malloc(sizeof(int64_t) * ((size_t)win_total + 1));
        void* pc = nullptr;
        if (plan_out.pieces.size() == 1 && plan_out.pieces[0].pc) { pc = plan_out.pieces[0].pc; plan_out.pieces[0].pc = nullptr; }      // one slice: its buffer is the result
        else {
            pc = result_alloc(sizeof(mhip_cns_piece) * (size_t)total, num_threads);
            size_t po = 0;
            if (pc) for (const PlanPiece& p : plan_out.pieces) {
                if (!p.pb) continue;
                const size_t bytes = sizeof(mhip_cns_piece) * (size_t)p.pb[p.nwin], part = (size_t)64 << 20;
                parallel_for((int64_t)((bytes + part - 1) / part), num_threads, [&](int64_t k) {
                    const size_t o = (size_t)k * part;
                    memcpy((char*)pc + po + o, (const char*)p.pc + o, std::min(part, bytes - o));
                });
                po += bytes;
            }
        }
        if (!pb || !pc) { free(pb); mhip_cns_free(pc); mhip_set_error("out of memory (%lld pieces)", (long long)total); return -1; }
        int64_t wo = 0, base = 0;
        for (const PlanPiece& p : plan_out.pieces) {
            for (int64_t i = 0; i < p.nwin; ++i) pb[wo + i] = base + (p.pb ? p.pb[i] : 0);
            wo += p.nwin;
            if (p.pb) base += p.pb[p.nwin];
        }
        pb[wo] = base;                          // (wo == win_total)
        *out_pc = pc; *out_pb = pb;
        return 0;
    };
    // the windows' consensus strings: every slice's bytes behind one another, cns_begin moved from slice-local to batch-wide offsets
    auto hand_over_poa = [&](char** out_cn, int64_t** out_cb) -> int {
        int64_t total = 0;
        for (const PlanPiece& p : plan_out.pieces) {
            if (p.pc_bad) { mhip_set_error("cns pieces: an index left its array, or the pieces written are not the pieces counted"); return -1; }
            if (p.cn_bad) { mhip_set_error("cns poa: a window's graph left its workspace bound, or a piece leaves its backbone"); return -1; }
            if (!p.cb) continue;
            const int64_t n = p.cb[p.nwin];
            if (p.cb[0] != 0 || n < 0 || n > p.cn_cap) { mhip_set_error("cns poa: inconsistent counts (%lld bytes in %lld)", (long long)n, (long long)p.cn_cap); return -1; }
            total += n;
        }
        int64_t* cb = (int64_t*)malloc(sizeof(int64_t) * ((size_t)win_total + 1));
        char* cn = (char*)result_alloc((size_t)total, num_threads);
        if (!cb || !cn) { free(cb); mhip_cns_free(cn); mhip_set_error("out of memory (%lld bytes of consensus)", (long long)total); return -1; }
        int64_t wo = 0, base = 0;
        for (const PlanPiece& p : plan_out.pieces) {
            for (int64_t i = 0; i < p.nwin; ++i) cb[wo + i] = base + (p.cb ? p.cb[i] : 0);
            wo += p.nwin;
            if (!p.cb) continue;
            const size_t bytes = (size_t)p.cb[p.nwin], part = (size_t)64 << 20;
            parallel_for((int64_t)((bytes + part - 1) / part), num_threads, [&](int64_t k) {
                const size_t o = (size_t)k * part;
                memcpy(cn + base + o, (const char*)p.cn + o, std::min(part, bytes - o));
            });
            base += p.cb[p.nwin];
        }
        cb[wo] = base;                          // (wo == win_total)
        *out_cn = cn; *out_cb = cb;
        return 0;
    };
    auto hand_over_plan = [&]() -> int {          // (after the last copy has landed)
        const size_t n1 = (size_t)num_templates + 1;
        for (const PlanPiece& p : plan_out.pieces)
            if (p.bad) { mhip_set_error("cns plan: the windows written are not the windows counted"); return -1; }
        void* pcs = nullptr;
        int64_t* pcb = nullptr;
        if (want_pieces && hand_over_pieces(&pcs, &pcb)) return -1;
        char* cns = nullptr;
        int64_t* cnb = nullptr;
        if (want_poa && hand_over_poa(&cns, &cnb)) { mhip_cns_free(pcs); free(pcb); return -1; }
        int64_t* sb = (int64_t*)malloc(sizeof(int64_t) * n1);
        int64_t* eb = (int64_t*)malloc(sizeof(int64_t) * n1);
        int32_t* er = (int32_t*)malloc(std::max<size_t>(sizeof(int32_t) * ER.size(), 1));
        void *seg = nullptr, *win = nullptr;
        if (plan_out.pieces.size() == 1) {
            seg = plan_out.pieces[0].seg; win = plan_out.pieces[0].win;
            mhip_cns_free(plan_out.pieces[0].pc); mhip_cns_free(plan_out.pieces[0].pb);      // (pc: NULL when it became the result)
            mhip_cns_free(plan_out.pieces[0].cn); mhip_cns_free(plan_out.pieces[0].cb);
            plan_out.pieces.clear();
        } else {
            seg = result_alloc(sizeof(mhip_cns_segment) * (size_t)seg_total, num_threads);
            win = result_alloc(sizeof(mhip_cns_window) * (size_t)win_total, num_threads);
        }
        if (!sb || !eb || !er || !seg || !win) { free(sb); free(eb); free(er); mhip_cns_free(seg); mhip_cns_free(win); mhip_cns_free(pcs); free(pcb); mhip_cns_free(cns); free(cnb); mhip_set_error("out of memory"); return -1; }
        size_t so = 0, wo = 0;
        for (PlanPiece& p : plan_out.pieces) {
            const size_t sbytes = sizeof(mhip_cns_segment) * (size_t)p.nseg, wbytes = sizeof(mhip_cns_window) * (size_t)p.nwin, piece = (size_t)64 << 20;
            if (sbytes) memcpy((char*)seg + so, p.seg, sbytes);
            parallel_for((int64_t)((wbytes + piece - 1) / piece), num_threads, [&](int64_t pc) {
                const size_t o = (size_t)pc * piece;
                memcpy((char*)win + wo + o, (const char*)p.win + o, std::min(piece, wbytes - o));
            });
            so += sbytes; wo += wbytes;
        }
        memcpy(sb, SB.data(), sizeof(int64_t) * n1);
        eb[0] = 0;
        for (size_t t = 0; t + 1 < n1; ++t) eb[t + 1] = eb[t] + ERB[t + 1];
        if (!ER.empty()) memcpy(er, ER.data(), sizeof(int32_t) * ER.size());
        *plan.seg = (mhip_cns_segment*)seg; *plan.seg_begin = sb; *plan.win = (mhip_cns_window*)win; *plan.n_win = win_total; *plan.er = er; *plan.er_begin = eb;
        if (want_pieces) { *plan.pc = (mhip_cns_piece*)pcs; *plan.pc_begin = pcb; }
        if (want_poa) { *plan.cns = cns; *plan.cns_begin = cnb; }
        return 0;
    };
    auto hand_over = [&]() -> int {
        if (want_tab && hand_over_tables()) return -1;
        const double t_put = now();
        const int plan_rc = want_plan ? hand_over_plan() : 0;
        tk[7] += now() - t_put;
        if (plan_rc) {
            if (want_tab) { mhip_cns_free(*out_table); mhip_cns_free(*out_ident); mhip_cns_free(*out_table_begin); *out_table = nullptr; *out_ident = nullptr; *out_table_begin = nullptr; }
            return -1;
        }
        return 0;
    };

    lap(0);
    // 2. the first <= 200 candidates of every template, as alignment jobs
    std::vector<int64_t> jfirst((size_t)num_templates + 1, 0);
    for (int t = 0; t < num_templates; ++t) jfirst[(size_t)t + 1] = jfirst[(size_t)t] + std::min<int64_t>(max_ext, tmpl_begin[t + 1] - tmpl_begin[t]);
    const int64_t nj = jfirst[(size_t)num_templates];
    if (out_jobs) *out_jobs = nj;
    if (nj == 0) return hand_over();
    if (nj > 0x7fffffffLL) { mhip_set_error("cns accept: too many jobs in one batch"); return -1; }
    std::vector<mhip_aln_job> jobs((size_t)nj);
    parallel_for(num_templates, num_threads, [&](int64_t t) {
        for (int64_t k = 0; k < jfirst[(size_t)t + 1] - jfirst[(size_t)t]; ++k) {
            const mhip_ext_candidate& ec = cands[tmpl_begin[t] + k];
            mhip_aln_job j;
            j.qid_local = ec.qid - start_id;
            j.sid_local = ec.sid - start_id;
            j.chain = ec.qdir != 0;
            j.qstart = ec.qdir != 0 ? ec.qsize - 1 - ec.qext : ec.qext;      // :428-429
            j.sstart = ec.sext;
            jobs[(size_t)(jfirst[(size_t)t] + k)] = j;
        }
    });
    int max_len = 16;
    for (int64_t i = 0; i < nj; ++i)
        max_len = std::max(max_len, std::max(vol->h_offs[(size_t)jobs[(size_t)i].qid_local].size, vol->h_offs[(size_t)jobs[(size_t)i].sid_local].size));
    // columns of one direction <= bases of both reads on that side; 16-column words
    const int cap = (int)(((int64_t)max_len * 2 + 64 + 15) / 16 * 16);
    const int row_words = 2 * (cap / 16);

    // 3. The batch goes through the device in SLICES of whole templates (at most MECAT_CNS_SLICE_JOBS jobs, default 1.2 M: four slices
    // at config 2) with two sets of buffers in turn:
    //     slice k + 1 is re-aligned on the GPU      while   a host thread replays the accept decisions of slice k
    //     the strings of slice k are built on the GPU behind it, and cross the PCIe link on a second stream while slice k + 2 re-aligns
    // The host side is the replay only; the string buffer is filled by the copy engine.
    int64_t slice_jobs = 1200000;
    if (const char* e = getenv("MECAT_CNS_SLICE_JOBS")) slice_jobs = std::max<int64_t>(1, atoll(e));
    std::vector<int> sl_t;                                    // first template of every slice, and one behind the last
    for (int t = 0; t < num_templates;) {
        sl_t.push_back(t);
        int u = t + 1;
        while (u < num_templates && jfirst[(size_t)u + 1] - jfirst[(size_t)t] <= slice_jobs) ++u;
        t = u;
    }
    sl_t.push_back(num_templates);
    const int nslices = (int)sl_t.size() - 1;
    int64_t max_slice = 0;
    for (int k = 0; k < nslices; ++k) max_slice = std::max(max_slice, jfirst[(size_t)sl_t[(size_t)k + 1]] - jfirst[(size_t)sl_t[(size_t)k]]);

    mhip_aln_job* d_jobs;
    if (c->scratch("ca_jobs", sizeof(mhip_aln_job) * (size_t)nj, (void**)&d_jobs)) return -1;
    HIPCHK(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(mhip_aln_job) * (size_t)nj, hipMemcpyHostToDevice, c->stream));
    mhip_cns_result* d_res[2] = {nullptr, nullptr};
    uint32_t* d_ops[2] = {nullptr, nullptr};
    for (int b = 0; b < std::min(2, nslices); ++b) {
        if (c->scratch(b ? "ca_res1" : "ca_res", sizeof(mhip_cns_result) * (size_t)max_slice, (void**)&d_res[b])) return -1;
        if (c->scratch(b ? "ca_ops1" : "ca_ops", sizeof(uint32_t) * (size_t)row_words * (size_t)max_slice, (void**)&d_ops[b])) return -1;
    }
    std::vector<mhip_cns_result> res((size_t)nj);           // every slice's results land in their place
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_built[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
    struct Cleanup {
        hipStream_t& s; hipEvent_t* a; hipEvent_t* b;
        ~Cleanup() {
            if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
            for (int i = 0; i < 2; ++i) { if (a[i]) (void)hipEventDestroy(a[i]); if (b[i]) (void)hipEventDestroy(b[i]); }
        }
    } cleanup{copy_stream, ev_built, ev_copied};
    HIPCHK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
        HIPCHK(hipEventCreateWithFlags(&ev_built[b], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_copied[b], hipEventDisableTiming));
    }

    // the result buffer: sized after the first slice's replay from its bytes per template (+ 15 %); a later slice that does not fit
    // gets a larger one, the strings copied so far moved over (MECAT_CNS_STR_ESTIMATE=<percent> scales the estimate: test knob)
    char* S = nullptr;
    size_t S_cap = 0, S_used = 0;
    bool S_big = false;
    auto s_release = [&]() {
        if (S && copy_stream) (void)hipStreamSynchronize(copy_stream);      // no copy may still be writing into it
        if (S) { if (S_big) mhip_cns_free(S); else free(S); }
        S = nullptr; S_cap = 0;
    };
    struct SGuard { std::function<void()> f; bool armed = true; ~SGuard() { if (armed) f(); } } s_guard{s_release};
    auto s_reserve = [&](size_t want) -> int {
        if (want <= S_cap) return 0;
        if (hipStreamSynchronize(copy_stream) != hipSuccess) { mhip_set_error("cns accept: copy stream failed"); return -1; }      // the copies into the old buffer have landed
        const bool big = want >= ((size_t)64 << 20);
        char* nS = big ? strbuf_get(want, num_threads) : (char*)malloc(std::max<size_t>(want, 1));
        if (!nS) { mhip_set_error("out of memory (%lld bytes of aligned strings)", (long long)want); return -1; }
        if (S_used) {
            const size_t piece = (size_t)64 << 20;
            parallel_for((int64_t)((S_used + piece - 1) / piece), num_threads, [&](int64_t pc) {
                const size_t o = (size_t)pc * piece;
                memcpy(nS + o, S + o, std::min(piece, S_used - o));
            });
        }
        s_release();
        S = nS; S_cap = want; S_big = big;
        return 0;
    };
    if (TW > 0) {
        tab_out.tab = (uint32_t*)result_alloc(sizeof(uint32_t) * (size_t)TW, num_threads);
        tab_out.id = (uint8_t*)result_alloc((size_t)TW, num_threads);
        if (!tab_out.tab || !tab_out.id) { mhip_set_error("out of memory (%lld table positions)", (long long)TW); return -1; }
    }
    double est_scale = 1.15;
    if (const char* e = getenv("MECAT_CNS_STR_ESTIMATE")) est_scale = std::max(0.01, atof(e) / 100.0);

    struct Slice {
        int t0 = 0, t1 = 0;
        int64_t j0 = 0, nj = 0;
        std::vector<std::vector<int32_t>> acc;      // per template: accepted job indices (batch-wide), in acceptance order
        std::vector<int64_t> afirst;               // per template: first accepted record of the slice
        std::vector<CnsStrItem> items;
        size_t sbytes = 0;
        std::vector<std::vector<int32_t>> er;      // per template: effective ranges, (start, end) pairs (with the plan only)
    };
    std::vector<mhip_cns_accepted> Avec;
    lap(1);

    auto align_slice = [&](Slice& sl, int b) -> int {
        if (mhip_cns_align_candidates_dev(c, vol, vol, d_jobs + sl.j0, (int)sl.nj, error_rate, min_align_size, cap, d_res[b], d_ops[b])) return -1;
        HIPCHK(hipMemcpyAsync(res.data() + sl.j0, d_res[b], sizeof(mhip_cns_result) * (size_t)sl.nj, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return 0;
    };
    // the sequential accept decisions, per template (host threads)
    auto replay_slice = [&](Slice& sl) {
        const int nt = sl.t1 - sl.t0;
        sl.acc.assign((size_t)nt, std::vector<int32_t>());
        sl.er.assign((size_t)(want_plan ? nt : 0), std::vector<int32_t>());
        parallel_for(nt, num_threads, [&](int64_t tl) {
            const int64_t t = sl.t0 + tl;
            const int64_t b = tmpl_begin[t], n = tmpl_begin[t + 1] - b;
            if (n == 0) return;
            const int ssize = vol->h_offs[(size_t)(cands[b].sid - start_id)].size;      // (== every candidate's ssize: checked above)
            std::vector<uint8_t> cov((size_t)std::max(ssize, 1), 0);
            std::set<int> used;
            int num_added = 0, num_ext = 0;
            for (int64_t i = 0; i < n && num_added < max_added && num_ext < max_ext; ++i) {
                ++num_ext;
                const mhip_ext_candidate& ec = cands[b + i];
                if (used.find(ec.qid) != used.end()) continue;
                const int64_t ji = jfirst[(size_t)t] + i;          // i < max_ext here: the job exists
                const mhip_cns_result& r = res[(size_t)ji];
                if (!r.ok) continue;
                const int oq = r.qend - r.qoff, qqs = (int)(ec.qsize * ratio), os = r.send - r.soff, qss = (int)(ec.ssize * ratio);      // :191-200
                if (!(oq >= qqs || os >= qss)) continue;
                int full = 0;                                        // check_cov_stats, :372-386
                for (int p = r.soff; p < r.send; ++p) full += cov[(size_t)p] >= 20;
                if (!(r.send - r.soff >= full + 200)) continue;
                for (int p = r.soff; p < r.send; ++p) ++cov[(size_t)p];
                ++num_added;
                used.insert(ec.qid);
                sl.acc[(size_t)tl].push_back((int32_t)ji);
            }
            if (want_plan) {                                         // cns_vec.get_mapping_ranges + get_effective_ranges, :445-447 (tech 1: :509)
                std::vector<std::pair<int32_t, int32_t>> mr;
                for (const int32_t ji : sl.acc[(size_t)tl]) mr.emplace_back(res[(size_t)ji].soff, res[(size_t)ji].send);
                cns_effective_ranges(mr, ssize, tech, plan.min_size, sl.er[(size_t)tl]);
            }
        });
        sl.afirst.assign((size_t)nt + 1, 0);
        for (int tl = 0; tl < nt; ++tl) sl.afirst[(size_t)tl + 1] = sl.afirst[(size_t)tl] + (int64_t)sl.acc[(size_t)tl].size();
        const int64_t na = sl.afirst[(size_t)nt];
        sl.items.resize((size_t)na);
        size_t off = 0;
        for (int tl = 0; tl < nt; ++tl)
            for (size_t k = 0; k < sl.acc[(size_t)tl].size(); ++k) {
                const int64_t ji = sl.acc[(size_t)tl][k];
                const mhip_cns_result& r = res[(size_t)ji];
                CnsStrItem& it = sl.items[(size_t)(sl.afirst[(size_t)tl] + (int64_t)k)];
                it.job = (int32_t)(ji - sl.j0);
                it.aln_size = r.last_col - r.first_col;          // O(ND) columns are matches or indels: normalising adds no columns
                it.off = (unsigned long long)off;
                off += 2 * ((size_t)it.aln_size + 1);
            }
        sl.sbytes = off;
    };
    // strings of an (aligned, replayed) slice: built on the device behind whatever the stream holds, copied on the second stream; the
    // slice's tables (whole templates: a contiguous piece of the output) zeroed, tallied from the strings and finished behind them
    auto strings_slice = [&](Slice& sl, int b, int k) -> int {
        const int64_t na = (int64_t)sl.items.size();
        const int64_t tw0 = build_tab ? TB[(size_t)sl.t0] : 0, tw = build_tab ? TB[(size_t)sl.t1] - tw0 : 0;
        if (want_plan) for (int t = sl.t0; t <= sl.t1; ++t) SB[(size_t)t] = seg_total;      // (what a slice without a table leaves)
        if (na == 0 && tw == 0) return 0;
        if (want_str && na) {
            size_t want = S_used + sl.sbytes;
            if (want > S_cap && k + 1 < nslices)
                want = std::max(want, (size_t)((double)want / (double)sl.t1 * (double)num_templates * est_scale) + ((size_t)1 << 20));
            if (s_reserve(want)) return -1;
        }
        std::vector<CnsTabItem> titems((size_t)(build_tab ? na : 0));
        // the accepted records (what the caller gets beside the strings)
        const size_t a0 = Avec.size();
        Avec.resize(a0 + (size_t)na);
        parallel_for(sl.t1 - sl.t0, num_threads, [&](int64_t tl) {
            const int64_t t = sl.t0 + tl;
            for (size_t kk = 0; kk < sl.acc[(size_t)tl].size(); ++kk) {
                const int64_t ji = sl.acc[(size_t)tl][kk];
                const mhip_cns_result& r = res[(size_t)ji];
                const CnsStrItem& it = sl.items[(size_t)(sl.afirst[(size_t)tl] + (int64_t)kk)];
                const mhip_ext_candidate& ec = cands[tmpl_begin[t] + (ji - jfirst[(size_t)t])];
                mhip_cns_accepted& o = Avec[a0 + (size_t)(sl.afirst[(size_t)tl] + (int64_t)kk)];
                o.template_index = (int32_t)t;
                o.cand_index = tmpl_begin[t] + (ji - jfirst[(size_t)t]);
                o.qid = ec.qid; o.sid = ec.sid;
                o.qoff = r.qoff; o.qend = r.qend; o.soff = r.soff; o.send = r.send;
                o.aln_size = it.aln_size;
                o.str_offset = want_str ? (int64_t)(S_used + it.off) : -1;
                if (build_tab) {
                    CnsTabItem& ti = titems[(size_t)(sl.afirst[(size_t)tl] + (int64_t)kk)];
                    ti.off = it.off; ti.tab = (unsigned long long)(TB[(size_t)t] - tw0); ti.aln_size = it.aln_size; ti.soff = r.soff;
                    ti.tab_len = (int32_t)(TB[(size_t)t + 1] - TB[(size_t)t]); ti.pad = 0;
                }
            }
        });
        if (k >= 2) HIPCHK(hipEventSynchronize(ev_copied[b]));      // the copies out of this set's buffers two slices ago (the string buffer may move)
        // (that slice's host arrays are done with now: this slice's take their place)
        hold_items[b].swap(sl.items);
        hold_titems[b].swap(titems);
        char* d_str = nullptr;
        if (na) {
            CnsStrItem* d_items;
            if (c->scratch(b ? "ca_str1" : "ca_str", sl.sbytes + 128, (void**)&d_str)) return -1;
            if (c->scratch(b ? "ca_items1" : "ca_items", sizeof(CnsStrItem) * (size_t)na, (void**)&d_items)) return -1;
            HIPCHK(hipMemcpyAsync(d_items, hold_items[b].data(), sizeof(CnsStrItem) * (size_t)na, hipMemcpyHostToDevice, c->stream));
            if (cns_strings_launch(c, vol, d_jobs + sl.j0, d_res[b], d_ops[b], row_words, d_items, (int)na, d_str)) return -1;
        }
        uint32_t* d_tab = nullptr;
        uint8_t* d_id = nullptr;
        if (tw) {
            std::vector<long long>& first = hold_first[b];
            std::vector<int32_t>& voloff = hold_voloff[b];
            first.clear(); voloff.clear();
            for (int t = sl.t0; t < sl.t1; ++t)
                if (TB[(size_t)t + 1] > TB[(size_t)t]) {
                    first.push_back((long long)(TB[(size_t)t] - tw0));
                    voloff.push_back(vol->h_offs[(size_t)(cands[tmpl_begin[t]].sid - start_id)].offset);
                }
            const int ntm = (int)voloff.size();
            first.push_back((long long)tw);
            CnsTabItem* d_titems;
            long long* d_first;
            int32_t* d_voloff;
            if (c->scratch(b ? "ca_tab1" : "ca_tab", sizeof(uint32_t) * (size_t)tw, (void**)&d_tab)) return -1;
            if (c->scratch(b ? "ca_ident1" : "ca_ident", (size_t)tw, (void**)&d_id)) return -1;
            if (c->scratch(b ? "ca_titems1" : "ca_titems", sizeof(CnsTabItem) * (size_t)std::max<int64_t>(na, 1), (void**)&d_titems)) return -1;
            if (c->scratch(b ? "ca_tfirst1" : "ca_tfirst", sizeof(long long) * ((size_t)ntm + 1), (void**)&d_first)) return -1;
            if (c->scratch(b ? "ca_tvoloff1" : "ca_tvoloff", sizeof(int32_t) * (size_t)ntm, (void**)&d_voloff)) return -1;
            if (na) HIPCHK(hipMemcpyAsync(d_titems, hold_titems[b].data(), sizeof(CnsTabItem) * (size_t)na, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_first, first.data(), sizeof(long long) * ((size_t)ntm + 1), hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_voloff, voloff.data(), sizeof(int32_t) * (size_t)ntm, hipMemcpyHostToDevice, c->stream));
            if (cns_table_launch(c, vol, d_str, d_titems, (int)na, d_tab, d_id, (long long)tw, d_first, d_voloff, ntm, nullptr)) return -1;
        }
        // the slice's plan, behind cns_table_finish on the same stream and in front of the copies
        CnsPlanDev pd;
        CnsPiecesDev qd;
        CnsPoaDev od;
        PlanPiece piece;
        if (want_plan && tw) {
            const int nt = sl.t1 - sl.t0;
            std::vector<long long> tbl((size_t)nt + 1), rbl((size_t)nt + 1, 0);
            std::vector<int32_t> erl;
            for (int tl = 0; tl <= nt; ++tl) tbl[(size_t)tl] = (long long)(TB[(size_t)(sl.t0 + tl)] - tw0);
            for (int tl = 0; tl < nt; ++tl) {
                erl.insert(erl.end(), sl.er[(size_t)tl].begin(), sl.er[(size_t)tl].end());
                rbl[(size_t)tl + 1] = (long long)(erl.size() / 2);
                ERB[(size_t)(sl.t0 + tl) + 1] = (int64_t)(sl.er[(size_t)tl].size() / 2);
            }
            ER.insert(ER.end(), erl.begin(), erl.end());
            if (cns_plan_launch(c, b, d_tab, d_id, nt, sl.t0, tbl.data(), erl.data(), rbl.data(), plan.min_cov, min_run, seg_total, win_total, SB.data() + sl.t0, &pd)) return -1;
            tk[6] += pd.wait_s;
            piece.nseg = pd.nseg; piece.nwin = pd.nwin;
            piece.seg = result_alloc(sizeof(mhip_cns_segment) * (size_t)pd.nseg, num_threads);
            piece.win = result_alloc(sizeof(mhip_cns_window) * (size_t)pd.nwin, num_threads);
            plan_out.pieces.push_back(piece);
            if (!piece.seg || !piece.win) { mhip_set_error("out of memory (%lld windows)", (long long)pd.nwin); return -1; }
            // the windows' pieces, behind cns_plan_emit on the same stream and in front of the copies: the slice's strings and plan are in place
            if ((want_pieces || want_poa) && pd.nwin > 0 && na > 0) {
                std::vector<CnsPieceItem> pitems((size_t)na);
                std::vector<long long> afl((size_t)nt + 1);
                for (int tl = 0; tl <= nt; ++tl) afl[(size_t)tl] = (long long)sl.afirst[(size_t)tl];
                parallel_for(nt, num_threads, [&](int64_t tl) {
                    for (int64_t i = sl.afirst[(size_t)tl]; i < sl.afirst[(size_t)tl + 1]; ++i) {
                        const mhip_cns_accepted& o = Avec[a0 + (size_t)i];
                        CnsPieceItem& it = pitems[(size_t)i];
                        it.off = hold_items[b][(size_t)i].off; it.aln_size = o.aln_size; it.soff = o.soff; it.send = o.send; it.tl = (int32_t)tl;
                    }
                });
                if (cns_pieces_launch(c, b, d_str, pitems.data(), na, (long long)a0, nt, sl.t0, afl.data(), tbl.data(), pd.d_seg, pd.nseg, pd.d_segb, seg_total, win_total, pd.d_win,
                                      pd.nwin, &qd)) return -1;
                tk[6] += qd.wait_s;
                PlanPiece& pp = plan_out.pieces.back();
                if (want_pieces) {
                    pp.pc_cap = qd.cap;
                    pp.pc = result_alloc(sizeof(mhip_cns_piece) * (size_t)qd.cap, num_threads);
                    pp.pb = (int64_t*)result_alloc(sizeof(int64_t) * ((size_t)pd.nwin + 1), num_threads);
                    if (!pp.pc || !pp.pb) { mhip_set_error("out of memory (%lld pieces)", (long long)qd.cap); return -1; }
                }
                // the windows' consensus, behind cns_pieces_emit on the same stream: the pieces stay where they are
                if (want_poa) {
                    if (cns_poa_launch(c, b, d_str, qd, na, (long long)a0, pd.d_win, pd.nwin, &od)) return -1;
                    tk[6] += od.wait_s;
                    poa_large += od.nlarge; poa_chunks += od.nchunks;
                    pp.cn_cap = od.cap;
                    pp.cn = result_alloc((size_t)od.cap, num_threads);
                    pp.cb = (int64_t*)result_alloc(sizeof(int64_t) * ((size_t)pd.nwin + 1), num_threads);
                    if (!pp.cn || !pp.cb) { mhip_set_error("out of memory (%lld bytes of consensus)", (long long)od.cap); return -1; }
                }
            }
            seg_total += pd.nseg; win_total += pd.nwin;
        }
        HIPCHK(hipEventRecord(ev_built[b], c->stream));
        HIPCHK(hipStreamWaitEvent(copy_stream, ev_built[b], 0));
        if (want_str && na) {
            HIPCHK(hipMemcpyAsync(S + S_used, d_str, sl.sbytes, hipMemcpyDeviceToHost, copy_stream));
            S_used += sl.sbytes;
        }
        if (pd.nseg) HIPCHK(hipMemcpyAsync(piece.seg, pd.d_seg, sizeof(mhip_cns_segment) * (size_t)pd.nseg, hipMemcpyDeviceToHost, copy_stream));
        if (pd.nwin) HIPCHK(hipMemcpyAsync(piece.win, pd.d_win, sizeof(mhip_cns_window) * (size_t)pd.nwin, hipMemcpyDeviceToHost, copy_stream));
        if (pd.d_bad) HIPCHK(hipMemcpyAsync(&plan_out.pieces.back().bad, pd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, copy_stream));      // (pieces: reserved, nothing moves)
        if (qd.d_pb) {                          // (the slots the bound allows; how many hold records is pb[nwin], read at the hand-over)
            PlanPiece& pp = plan_out.pieces.back();
            if (want_pieces) {
                if (qd.cap) HIPCHK(hipMemcpyAsync(pp.pc, qd.d_pieces, sizeof(mhip_cns_piece) * (size_t)qd.cap, hipMemcpyDeviceToHost, copy_stream));
                HIPCHK(hipMemcpyAsync(pp.pb, qd.d_pb, sizeof(int64_t) * ((size_t)pd.nwin + 1), hipMemcpyDeviceToHost, copy_stream));
            }
            HIPCHK(hipMemcpyAsync(&pp.pc_bad, qd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, copy_stream));
        }
        if (od.d_cb) {                          // (the bytes the bound allows; how many hold strings is cb[nwin], read at the hand-over)
            PlanPiece& pp = plan_out.pieces.back();
            if (od.cap) HIPCHK(hipMemcpyAsync(pp.cn, od.d_cns, (size_t)od.cap, hipMemcpyDeviceToHost, copy_stream));
            HIPCHK(hipMemcpyAsync(pp.cb, od.d_cb, sizeof(int64_t) * ((size_t)pd.nwin + 1), hipMemcpyDeviceToHost, copy_stream));
            HIPCHK(hipMemcpyAsync(&pp.cn_bad, od.d_bad, sizeof(long long), hipMemcpyDeviceToHost, copy_stream));
        }
        if (tw && want_tab) {
            HIPCHK(hipMemcpyAsync(tab_out.tab + tw0, d_tab, sizeof(uint32_t) * (size_t)tw, hipMemcpyDeviceToHost, copy_stream));
            HIPCHK(hipMemcpyAsync(tab_out.id + tw0, d_id, (size_t)tw, hipMemcpyDeviceToHost, copy_stream));
        }
        HIPCHK(hipEventRecord(ev_copied[b], copy_stream));
        return 0;
    };

    std::vector<Slice> slices((size_t)nslices);
    plan_out.pieces.reserve((size_t)nslices);
    for (int k = 0; k < nslices; ++k) {
        Slice& sl = slices[(size_t)k];
        sl.t0 = sl_t[(size_t)k]; sl.t1 = sl_t[(size_t)k + 1];
        sl.j0 = jfirst[(size_t)sl.t0]; sl.nj = jfirst[(size_t)sl.t1] - sl.j0;
    }
    if (slices[0].nj > 0 && align_slice(slices[0], 0)) return -1;
    lap(2);
    for (int k = 0; k < nslices; ++k) {
        Slice& sl = slices[(size_t)k];
        std::thread rp([&]() { replay_slice(sl); });
        struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } } join{rp};
        int rc = 0;
        if (k + 1 < nslices && slices[(size_t)k + 1].nj > 0) rc = align_slice(slices[(size_t)k + 1], (k + 1) & 1);
        lap(2);
        rp.join();
        lap(3);
        if (rc) return -1;
        if (strings_slice(sl, k & 1, k)) return -1;
        sl.acc.clear(); sl.acc.shrink_to_fit(); sl.items.clear(); sl.items.shrink_to_fit();
        lap(4);
    }
    HIPCHK(hipStreamSynchronize(copy_stream));
    const int64_t na = (int64_t)Avec.size();
    if (na == 0) return hand_over();
    mhip_cns_accepted* A = (mhip_cns_accepted*)malloc(sizeof(mhip_cns_accepted) * (size_t)na);
    if (!A) { mhip_set_error("out of memory"); return -1; }
    memcpy(A, Avec.data(), sizeof(mhip_cns_accepted) * (size_t)na);
    if (hand_over()) { free(A); return -1; }
    const int64_t sbytes = (int64_t)S_used;
    s_guard.armed = false;
    lap(5);
    if (times)
        fprintf(stderr, "[cns_accept] %d templates, %lld jobs in %d slices, %lld accepted, %.2f GB of strings: sort + checks %.3f s, jobs %.3f, re-alignment on the "
                        "device %.3f, accept replay beyond it %.3f, strings launched %.3f, last copies %.3f\n", num_templates, (long long)nj, nslices, (long long)na,
                (double)sbytes / 1e9, tk[0], tk[1], tk[2], tk[3], tk[4], tk[5]);
    if (times && want_pieces)
        fprintf(stderr, "[cns_accept] pieces: %lld pieces (the waits for their bound are counted with the plan's)\n", (long long)(*plan.pc_begin)[win_total]);
    if (times && want_poa)
        fprintf(stderr, "[cns_accept] poa: %lld bytes of consensus, %lld windows in cns_poa_large (%lld launches); the waits for the bounds are counted with the plan's\n",
                (long long)(*plan.cns_begin)[win_total], poa_large, poa_chunks);
    if (times && want_plan)
        fprintf(stderr, "[cns_accept] plan: %lld segments, %lld windows: waited for the counts %.3f s (within strings launched), slices' pieces put together %.3f (within last copies)\n",
                (long long)seg_total, (long long)win_total, tk[6], tk[7]);
    *out_accepted = A;
    *out_count = na;
    *out_strings = S;
    *out_strings_bytes = sbytes;
    return 0;
}

int mhip_cns_accept_templates(mhip_ctx* c, const mhip_volume* vol, const uint8_t* /*host_pac: not read any more (the strings are built on the device)*/, mhip_ext_candidate* cands, const int64_t* tmpl_begin,
                              int num_templates, int tech, int min_align_size, double min_mapping_ratio, int num_threads,
                              mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings, int64_t* out_strings_bytes,
                              int64_t* out_jobs) {
    return cns_accept_body(c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, true, false, out_accepted, out_count,
                           out_strings, out_strings_bytes, out_jobs, nullptr, nullptr, nullptr, PlanArgs());
}

int mhip_cns_accept_templates_ex(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, int tech,
                                 int min_align_size, double min_mapping_ratio, int num_threads, int want, mhip_cns_accepted** out_accepted, int64_t* out_count,
                                 char** out_strings, int64_t* out_strings_bytes, int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident,
                                 int64_t** out_table_begin) {
    const bool want_tab = (want & MHIP_CNS_WANT_TABLE) != 0;
    if (want == 0 || (want & ~(MHIP_CNS_WANT_STRINGS | MHIP_CNS_WANT_TABLE))) { mhip_set_error("cns accept: want = %d (MHIP_CNS_WANT_STRINGS | MHIP_CNS_WANT_TABLE)", want); return -1; }
    if (want_tab && (!out_table || !out_ident || !out_table_begin)) { mhip_set_error("cns accept: the table was asked for without a place to put it"); return -1; }
    if (out_table) *out_table = nullptr;
    if (out_ident) *out_ident = nullptr;
    if (out_table_begin) *out_table_begin = nullptr;
    return cns_accept_body(c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, (want & MHIP_CNS_WANT_STRINGS) != 0, want_tab,
                           out_accepted, out_count, out_strings, out_strings_bytes, out_jobs, out_table, out_ident, out_table_begin, PlanArgs());
}

// the body of mhip_cns_accept_templates_plan, _pieces and _poa; `allowed`: the bits of `want` the entry point takes
static int cns_accept_plan_entry(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, int tech,
                                 int min_align_size, double min_mapping_ratio, int num_threads, int want, int allowed, int min_cov, int min_size,
                                 mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings, int64_t* out_strings_bytes, int64_t* out_jobs,
                                 mhip_cns_table_item** out_table, uint8_t** out_ident, int64_t** out_table_begin, mhip_cns_segment** out_segments,
                                 int64_t** out_seg_begin, mhip_cns_window** out_windows, int64_t* out_n_windows, int32_t** out_eranges, int64_t** out_erange_begin,
                                 mhip_cns_piece** out_pieces, int64_t** out_piece_begin, char** out_cns, int64_t** out_cns_begin) {
    const bool want_tab = (want & MHIP_CNS_WANT_TABLE) != 0;
    PlanArgs plan;
    plan.want = (want & MHIP_CNS_WANT_PLAN) != 0;
    plan.want_pieces = (want & MHIP_CNS_WANT_PIECES) != 0;
    plan.want_poa = (want & MHIP_CNS_WANT_POA) != 0;
    if (want == 0 || (want & ~allowed)) {
        mhip_set_error("cns accept: want = %d (MHIP_CNS_WANT_STRINGS | MHIP_CNS_WANT_TABLE | MHIP_CNS_WANT_PLAN%s)", want, (allowed & MHIP_CNS_WANT_POA) ? " | MHIP_CNS_WANT_PIECES | MHIP_CNS_WANT_POA" : (allowed & MHIP_CNS_WANT_PIECES) ? " | MHIP_CNS_WANT_PIECES" : "");
        return -1;
    }
    if (plan.want_pieces && !plan.want) { mhip_set_error("cns accept: want = %d: MHIP_CNS_WANT_PIECES needs MHIP_CNS_WANT_PLAN (pieces belong to the plan's windows)", want); return -1; }
    if (plan.want_poa && !plan.want) { mhip_set_error("cns accept: want = %d: MHIP_CNS_WANT_POA needs MHIP_CNS_WANT_PLAN (the consensus belongs to the plan's windows)", want); return -1; }
    if (plan.want_poa && (!out_cns || !out_cns_begin)) { mhip_set_error("cns accept: the consensus was asked for without a place to put it"); return -1; }
    if (plan.want_pieces && (!out_pieces || !out_piece_begin)) { mhip_set_error("cns accept: the pieces were asked for without a place to put them"); return -1; }
    if (want_tab && (!out_table || !out_ident || !out_table_begin)) { mhip_set_error("cns accept: the table was asked for without a place to put it"); return -1; }
    if (plan.want && (!out_segments || !out_seg_begin || !out_windows || !out_n_windows || !out_eranges || !out_erange_begin)) {
        mhip_set_error("cns accept: the plan was asked for without a place to put it");
        return -1;
    }
    if (plan.want && (min_size < 2 || min_cov < 1)) { mhip_set_error("cns accept: the plan needs min_size >= 2 and min_cov >= 1 (%d, %d)", min_size, min_cov); return -1; }
    if (out_table) *out_table = nullptr;
    if (out_ident) *out_ident = nullptr;
    if (out_table_begin) *out_table_begin = nullptr;
    if (out_segments) *out_segments = nullptr;
    if (out_seg_begin) *out_seg_begin = nullptr;
    if (out_windows) *out_windows = nullptr;
    if (out_n_windows) *out_n_windows = 0;
    if (out_eranges) *out_eranges = nullptr;
    if (out_erange_begin) *out_erange_begin = nullptr;
    if (out_pieces) *out_pieces = nullptr;
    if (out_piece_begin) *out_piece_begin = nullptr;
    if (out_cns) *out_cns = nullptr;
    if (out_cns_begin) *out_cns_begin = nullptr;
    plan.pc = out_pieces; plan.pc_begin = out_piece_begin;
    plan.cns = out_cns; plan.cns_begin = out_cns_begin;
    plan.min_cov = min_cov; plan.min_size = min_size;
    plan.seg = out_segments; plan.seg_begin = out_seg_begin; plan.win = out_windows; plan.n_win = out_n_windows; plan.er = out_eranges; plan.er_begin = out_erange_begin;
    return cns_accept_body(c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, (want & MHIP_CNS_WANT_STRINGS) != 0, want_tab,
                           out_accepted, out_count, out_strings, out_strings_bytes, out_jobs, out_table, out_ident, out_table_begin, plan);
}

int mhip_cns_accept_templates_plan(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, int tech,
                                   int min_align_size, double min_mapping_ratio, int num_threads, int want, int min_cov, int min_size,
                                   mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings, int64_t* out_strings_bytes, int64_t* out_jobs,
                                   mhip_cns_table_item** out_table, uint8_t** out_ident, int64_t** out_table_begin, mhip_cns_segment** out_segments,
                                   int64_t** out_seg_begin, mhip_cns_window** out_windows, int64_t* out_n_windows, int32_t** out_eranges, int64_t** out_erange_begin) {
    return cns_accept_plan_entry(c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, want,
                                 MHIP_CNS_WANT_STRINGS | MHIP_CNS_WANT_TABLE | MHIP_CNS_WANT_PLAN, min_cov, min_size, out_accepted, out_count, out_strings, out_strings_bytes,
                                 out_jobs, out_table, out_ident, out_table_begin, out_segments, out_seg_begin, out_windows, out_n_windows, out_eranges, out_erange_begin,
                                 nullptr, nullptr, nullptr, nullptr);
}

int mhip_cns_accept_templates_pieces(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, int tech,
                                     int min_align_size, double min_mapping_ratio, int num_threads, int want, int min_cov, int min_size,
                                     mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings, int64_t* out_strings_bytes, int64_t* out_jobs,
                                     mhip_cns_table_item** out_table, uint8_t** out_ident, int64_t** out_table_begin, mhip_cns_segment** out_segments,
                                     int64_t** out_seg_begin, mhip_cns_window** out_windows, int64_t* out_n_windows, int32_t** out_eranges, int64_t** out_erange_begin,
                                     mhip_cns_piece** out_pieces, int64_t** out_piece_begin) {
    return cns_accept_plan_entry(c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, want,
                                 MHIP_CNS_WANT_STRINGS | MHIP_CNS_WANT_TABLE | MHIP_CNS_WANT_PLAN | MHIP_CNS_WANT_PIECES, min_cov, min_size, out_accepted, out_count, out_strings,
                                 out_strings_bytes, out_jobs, out_table, out_ident, out_table_begin, out_segments, out_seg_begin, out_windows, out_n_windows, out_eranges,
                                 out_erange_begin, out_pieces, out_piece_begin, nullptr, nullptr);
}

int mhip_cns_accept_templates_poa(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, int tech,
                                  int min_align_size, double min_mapping_ratio, int num_threads, int want, int min_cov, int min_size,
                                  mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings, int64_t* out_strings_bytes, int64_t* out_jobs,
                                  mhip_cns_table_item** out_table, uint8_t** out_ident, int64_t** out_table_begin, mhip_cns_segment** out_segments,
                                  int64_t** out_seg_begin, mhip_cns_window** out_windows, int64_t* out_n_windows, int32_t** out_eranges, int64_t** out_erange_begin,
                                  mhip_cns_piece** out_pieces, int64_t** out_piece_begin, char** out_cns, int64_t** out_cns_begin) {
    return cns_accept_plan_entry(c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, want,
                                 MHIP_CNS_WANT_STRINGS | MHIP_CNS_WANT_TABLE | MHIP_CNS_WANT_PLAN | MHIP_CNS_WANT_PIECES | MHIP_CNS_WANT_POA, min_cov, min_size, out_accepted,
                                 out_count, out_strings, out_strings_bytes, out_jobs, out_table, out_ident, out_table_begin, out_segments, out_seg_begin, out_windows,
                                 out_n_windows, out_eranges, out_erange_begin, out_pieces, out_piece_begin, out_cns, out_cns_begin);
}

}  // extern "C"
