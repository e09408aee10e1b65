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
// mhip_cns_accept_templates_poa adds the POA consensus of every listed window (meap_cns_one_indel, :62-78) — cns_poa.hip — and
// mhip_cns_accept_templates_reads what the reference ends with: every segment's target put together from the anchors' letters and the
// windows' strings (:88-107), the size filter and output_cns_result's records (:233, :155-188), behind a slice's consensus — cns_reads.hip.
// mhip_cns_correct_templates is the entry point of the mecat2cns program: the same stages with the options and outputs in two structs,
// the walk of consensus_one_read_m4_* (:241-360) as a second rule set in front of the strings (input_type 1: cns_replay.h), and the
// FASTA text of the records made on the device behind a slice's read kernels (reads_correction_can.cpp:44-46) — cns_text.hip.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "common.h"
#include "cns_hostbuf.h"
#include "cns_pieces.h"
#include "cns_plan.h"
#include "cns_poa_dev.h"
#include "cns_ranges.h"
#include "cns_reads.h"
#include "cns_replay.h"
#include "cns_slices.h"
#include "cns_strings.h"
#include "cns_table.h"
#include "cns_text.h"

namespace {

const int WANT_STR = MHIP_CNS_WANT_STRINGS, WANT_TAB = MHIP_CNS_WANT_TABLE, WANT_PLAN = MHIP_CNS_WANT_PLAN, WANT_PIECES = MHIP_CNS_WANT_PIECES, WANT_POA = MHIP_CNS_WANT_POA, WANT_READS = MHIP_CNS_WANT_READS, WANT_TEXT = MHIP_CNS_WANT_TEXT;

struct CmpByScore {      // CmpExtensionCandidateByScore, mecat_correction.cpp:362-370
    bool operator()(const mhip_ext_candidate& a, const mhip_ext_candidate& b) const {
        if (a.score != b.score) return a.score > b.score;
        if (a.qid != b.qid) return a.qid < b.qid;
        return a.qext < b.qext;
    }
};

// one call of any of the entry points: the inputs, the outputs asked for and where they go (NULL: the entry point has no such output)
struct AcceptCall {
    mhip_ctx* c; const mhip_volume* vol; mhip_ext_candidate* cands; const int64_t* tmpl_begin;
    int num_templates, tech, min_align_size; double min_mapping_ratio; int num_threads, want, min_cov, min_size;
    mhip_cns_accepted** accepted; int64_t* count; char** strings; int64_t* strings_bytes; int64_t* jobs;
    mhip_cns_table_item** table = nullptr; uint8_t** ident = nullptr; int64_t** table_begin = nullptr;
    mhip_cns_segment** segments = nullptr; int64_t** seg_begin = nullptr; mhip_cns_window** windows = nullptr; int64_t* n_windows = nullptr; int32_t** eranges = nullptr; int64_t** erange_begin = nullptr;
    mhip_cns_piece** pieces = nullptr; int64_t** piece_begin = nullptr; char** cns = nullptr; int64_t** cns_begin = nullptr;
    mhip_cns_read** reads = nullptr; int64_t** read_begin = nullptr; char** seq = nullptr; int64_t* seq_bytes = nullptr;
    int input_type = 0; char** text = nullptr; int64_t* text_bytes = nullptr;      // (mhip_cns_correct_templates only)
};

template <typename T> void clear_out(T* p) { if (p) *p = T(); }

// `allowed`: the bits of `want` the entry point takes.  Every output is NULL / 0 afterwards
int validate(const AcceptCall& a, int allowed) {
    const int want = a.want;
    const char *plan = (allowed & WANT_PLAN) ? " | MHIP_CNS_WANT_PLAN" : "", *pieces = (allowed & WANT_PIECES) ? " | MHIP_CNS_WANT_PIECES" : "", *poa = (allowed & WANT_POA) ? " | MHIP_CNS_WANT_POA" : "";
    const char *reads = (allowed & WANT_READS) ? " | MHIP_CNS_WANT_READS" : "", *text = (allowed & WANT_TEXT) ? " | MHIP_CNS_WANT_TEXT" : "";
    if (want == 0 || (want & ~allowed)) { mhip_set_error("cns accept: want = %d (MHIP_CNS_WANT_STRINGS | MHIP_CNS_WANT_TABLE%s%s%s%s%s)", want, plan, pieces, poa, reads, text); return -1; }
    if (a.input_type != 0 && a.input_type != 1) { mhip_set_error("cns accept: input_type = %d (0: the .can walk, 1: the m4 walk)", a.input_type); return -1; }
    if ((want & WANT_PIECES) && !(want & WANT_PLAN)) { mhip_set_error("cns accept: want = %d: MHIP_CNS_WANT_PIECES needs MHIP_CNS_WANT_PLAN (pieces belong to the plan's windows)", want); return -1; }
    if ((want & WANT_POA) && !(want & WANT_PLAN)) { mhip_set_error("cns accept: want = %d: MHIP_CNS_WANT_POA needs MHIP_CNS_WANT_PLAN (the consensus belongs to the plan's windows)", want); return -1; }
    if ((want & WANT_POA) && (!a.cns || !a.cns_begin)) { mhip_set_error("cns accept: the consensus was asked for without a place to put it"); return -1; }
    if ((want & WANT_PIECES) && (!a.pieces || !a.piece_begin)) { mhip_set_error("cns accept: the pieces were asked for without a place to put them"); return -1; }
    if ((want & WANT_TAB) && (!a.table || !a.ident || !a.table_begin)) { mhip_set_error("cns accept: the table was asked for without a place to put it"); return -1; }
    if ((want & WANT_PLAN) && (!a.segments || !a.seg_begin || !a.windows || !a.n_windows || !a.eranges || !a.erange_begin)) { mhip_set_error("cns accept: the plan was asked for without a place to put it"); return -1; }
    if ((want & WANT_READS) && (!a.reads || !a.read_begin || !a.seq || !a.seq_bytes)) { mhip_set_error("cns accept: the reads were asked for without a place to put them"); return -1; }
    if ((want & WANT_TEXT) && (!a.text || !a.text_bytes)) { mhip_set_error("cns accept: the text was asked for without a place to put it"); return -1; }
    if ((want & (WANT_PLAN | WANT_READS | WANT_TEXT)) && (a.min_size < 2 || a.min_cov < 1)) { mhip_set_error("cns accept: the plan needs min_size >= 2 and min_cov >= 1 (%d, %d)", a.min_size, a.min_cov); return -1; }
    clear_out(a.accepted); clear_out(a.count); clear_out(a.strings); clear_out(a.strings_bytes); clear_out(a.jobs); clear_out(a.table); clear_out(a.ident); clear_out(a.table_begin);
    clear_out(a.segments); clear_out(a.seg_begin); clear_out(a.windows); clear_out(a.n_windows); clear_out(a.eranges); clear_out(a.erange_begin);
    clear_out(a.pieces); clear_out(a.piece_begin); clear_out(a.cns); clear_out(a.cns_begin);
    clear_out(a.reads); clear_out(a.read_begin); clear_out(a.seq); clear_out(a.seq_bytes); clear_out(a.text); clear_out(a.text_bytes);
    return 0;
}

// MECAT_CNS_TIMES=1: where the call's wall time went, on stderr
enum Lap { LAP_SORT, LAP_JOBS, LAP_ALIGN, LAP_REPLAY, LAP_STRINGS, LAP_LAST_COPIES, LAP_PLAN_WAIT, LAP_PUT, LAP_COUNT };
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Slice {
    int t0 = 0, t1 = 0; int64_t j0 = 0, nj = 0;      // templates [t0, t1), jobs [j0, j0 + nj)
    std::vector<std::vector<int32_t>> acc;      // per template: accepted job indices (batch-wide), in acceptance order
    std::vector<int64_t> afirst;               // per template: first accepted record of the slice
    std::vector<CnsStrItem> items;
    size_t sbytes = 0;
    std::vector<std::vector<int32_t>> er;      // per template: effective ranges, (start, end) pairs (with the plan only)
};

// A slice's part of the plan, in host buffers of its own (the sizes are known slice by slice only), put together at the hand-over; the
// records are final when they leave the device.  win.bad is CnsPlanDev::d_bad: copied with the windows and looked at in the hand-over
// only, after every slice has run (an overflow of the segment slots is refused by cns_plan_launch at once).  pc: cns_pieces.hip's slots,
// cn: cns_poa.hip's bytes, both with begin[] per window of the slice.  rd, sq: cns_reads.hip's records and letters (counts the host knows)
// with tbegin[nt + 1], the first record of each of the slice's templates [t0, t0 + nt).  tx: cns_text.hip's bytes (a count the host knows).
struct PlanSlice { SliceOut seg, win, pc, cn, rd, sq, tx; CnsBuf<int64_t> tbegin; int t0 = 0, nt = 0; };

// the state of one call
struct Batch {
    const AcceptCall& a;
    mhip_ctx* const c;
    const bool want_str, want_tab, want_plan, want_pieces, want_poa, want_reads, want_text;
    // build_*: what the outputs asked for read is built on the device either way and copied only when asked for itself — the plan reads the
    // table, the reads read table, plan and consensus, the text reads the reads
    const bool build_reads, build_plan, build_pieces, build_poa, build_tab;
    const int threads, start_id, min_run;
    const CnsReplayRules rules;
    const CnsReplayM4Rules m4;                 // input_type 1
    const double error_rate;                   // mecat_correction.cpp:431 / :494
    double tk[LAP_COUNT] = {}, t_last = now();
    std::vector<int64_t> TB, jfirst;           // per template: first table word (one word per base of every template that has candidates); first job
    int64_t TW = 0, nj = 0;                    // table words that go to the caller; jobs
    std::vector<mhip_aln_job> jobs;
    int cap = 0, row_words = 0, nslices = 0;      // columns a direction may take, words of a job's two op rows
    mhip_aln_job* d_jobs = nullptr;
    mhip_cns_result* d_res[2] = {nullptr, nullptr}; uint32_t* d_ops[2] = {nullptr, nullptr};      // the two sets
    std::vector<mhip_cns_result> res;          // every slice's results land in their place
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_built[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
    // host buffers of the table outputs (filled by the copy stream), and the host arrays behind the slices' item copies: a set's arrays
    // live until the copies that follow the kernels which read them have completed
    CnsBuf<uint32_t> tab; CnsBuf<uint8_t> ident;
    std::vector<CnsStrItem> hold_items[2]; std::vector<CnsTabItem> hold_titems[2];
    std::vector<long long> hold_first[2]; std::vector<int32_t> hold_voloff[2];
    // the string buffer: sized after the first slice's replay from its bytes per template (+ 15 %); a later slice that does not fit
    // gets a larger one, the strings copied so far moved over (MECAT_CNS_STR_ESTIMATE=<percent> scales the estimate: test knob)
    CnsBuf<char> S;
    size_t S_cap = 0, S_used = 0;
    double est_scale = 1.15;
    std::vector<mhip_cns_accepted> Avec;
    std::vector<PlanSlice> plan;                  // the slices that had a table
    std::vector<int64_t> SB, ERB;                 // per template: first segment; effective ranges (counts until the hand-over)
    std::vector<int32_t> ER;
    int64_t seg_total = 0, win_total = 0;
    long long poa_large = 0, poa_chunks = 0;      // windows that went to cns_poa_large, and its launches
    double reads_wait = 0, text_wait = 0;         // host seconds in cns_reads_launch's and cns_text_launch's waits (counted with the plan's as well)
    int64_t reads_total = 0, seq_total = 0, text_total = 0;

    explicit Batch(const AcceptCall& a_)
        : a(a_), c(a_.c), want_str(a_.want & WANT_STR), want_tab(a_.want & WANT_TAB), want_plan(a_.want & WANT_PLAN), want_pieces(a_.want & WANT_PIECES), want_poa(a_.want & WANT_POA),
          want_reads(a_.want & WANT_READS), want_text(a_.want & WANT_TEXT), build_reads(want_reads || want_text), build_plan(want_plan || build_reads),
          build_pieces(want_pieces || want_poa || build_reads), build_poa(want_poa || build_reads),
          build_tab(want_tab || build_plan), threads(std::max(1, a_.num_threads)), start_id(a_.vol->start_read_id), min_run(build_plan ? cns_plan_min_run(a_.min_size) : 0),
          rules{200, a_.tech == 0 ? 60 : 100, a_.min_mapping_ratio - 0.02}, m4{a_.tech == 0 ? 60 : 100, a_.tech != 0, a_.min_mapping_ratio - 0.02},
          error_rate(a_.tech == 0 ? 0.15 : 0.20) {}
    // no copy may still be writing into a buffer that goes: the body runs before any member is released
    ~Batch() {
        if (copy_stream) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); }
        for (int i = 0; i < 2; ++i) { if (ev_built[i]) (void)hipEventDestroy(ev_built[i]); if (ev_copied[i]) (void)hipEventDestroy(ev_copied[i]); }
    }
    void lap(Lap k) { const double t = now(); tk[k] += t - t_last; t_last = t; }
    int read_size(int t) const { return a.vol->h_offs[(size_t)(a.cands[a.tmpl_begin[t]].sid - start_id)].size; }      // of a template that has candidates
};

// the order of the reference's walk, and what the call refuses in a candidate
int sort_and_check(Batch& b) {
    const AcceptCall& a = b.a;
    const int start_id = b.start_id, nreads = a.vol->num_reads;
    std::atomic<int> bad{0};
    parallel_for(a.num_templates, b.threads, [&](int64_t t) {
        mhip_ext_candidate *s = a.cands + a.tmpl_begin[t], *e = a.cands + a.tmpl_begin[t + 1];
        // std::sort, not stable_sort: the reference sorts the same array (file order of the partition) with the same comparator and
        // the same libstdc++ introsort (mecat_correction.cpp:409 / :472), so records that tie on (score, qid, qext) come out in the
        // reference's order exactly when the input order is the reference's — which is what the caller hands over
        if (a.input_type == 0) std::sort(s, e, CmpByScore());
        else cns_replay_m4_order(s, e - s, b.m4);      // (as given, or the whole range by overlap size: the same argument, cns_replay.h)
        for (mhip_ext_candidate* p = s; p < e; ++p) {
            if (p->sdir != 0 || p->qid < start_id || p->qid >= start_id + nreads || p->sid < start_id || p->sid >= start_id + nreads || p->sid != s->sid) { bad = 1; continue; }
            // the record's read lengths are the volume's: the replay indexes the coverage array and the reads with them (the
            // reference has a fixed MAX_SEQ_SIZE array there; a record that disagrees with the volume is refused, not trusted)
            if (p->qsize != a.vol->h_offs[(size_t)(p->qid - start_id)].size || p->ssize != a.vol->h_offs[(size_t)(p->sid - start_id)].size) bad = 2;
        }
    });
    if (bad.load() == 2) { mhip_set_error("cns accept: a candidate's qsize / ssize differs from the read lengths of the volume"); return -1; }
    if (bad.load()) { mhip_set_error("cns accept: a candidate is outside the volume, has sdir != 0 or sits in another template's range"); return -1; }
    return 0;
}

// the first <= 200 candidates (m4 walk: <= max_added overlaps) of every template, as alignment jobs
void make_jobs(Batch& b) {
    const AcceptCall& a = b.a;
    b.jobs.resize((size_t)b.nj);
    parallel_for(a.num_templates, b.threads, [&](int64_t t) {
        for (int64_t k = 0; k < b.jfirst[(size_t)t + 1] - b.jfirst[(size_t)t]; ++k) {
            const mhip_ext_candidate& ec = a.cands[a.tmpl_begin[t] + k];
            mhip_aln_job j;
            j.qid_local = ec.qid - b.start_id; j.sid_local = ec.sid - b.start_id; j.chain = ec.qdir != 0; j.sstart = ec.sext;
            j.qstart = ec.qdir != 0 ? ec.qsize - 1 - ec.qext : ec.qext;      // :428-429
            b.jobs[(size_t)(b.jfirst[(size_t)t] + k)] = j;
        }
    });
    int max_len = 16;
    for (const mhip_aln_job& j : b.jobs) max_len = std::max(max_len, std::max(a.vol->h_offs[(size_t)j.qid_local].size, a.vol->h_offs[(size_t)j.sid_local].size));
    // columns of one direction <= bases of both reads on that side; 16-column words
    b.cap = (int)(((int64_t)max_len * 2 + 64 + 15) / 16 * 16); b.row_words = 2 * (b.cap / 16);
}

// The batch goes through the device in SLICES of whole templates (at most MECAT_CNS_SLICE_JOBS jobs, default 1.2 M: four slices
// at config 2) with two sets of buffers in turn:
//     slice k + 1 is re-aligned on the GPU      while   a host thread replays the accept decisions of slice k
//     the strings of slice k are built on the GPU behind it, and cross the PCIe link on a second stream while slice k + 2 re-aligns
// The host side is the replay only; the string buffer is filled by the copy engine.
std::vector<Slice> cut_slices(const Batch& b) {
    int64_t slice_jobs = 1200000;
    if (const char* e = getenv("MECAT_CNS_SLICE_JOBS")) slice_jobs = std::max<int64_t>(1, atoll(e));
    std::vector<Slice> slices;
    for (int t = 0; t < b.a.num_templates;) {
        int u = t + 1;
        while (u < b.a.num_templates && b.jfirst[(size_t)u + 1] - b.jfirst[(size_t)t] <= slice_jobs) ++u;
        Slice sl;
        sl.t0 = t; sl.t1 = u; sl.j0 = b.jfirst[(size_t)t]; sl.nj = b.jfirst[(size_t)u] - sl.j0;
        slices.push_back(std::move(sl));
        t = u;
    }
    return slices;
}

// the jobs on the device, the two sets of result buffers, the copy stream and its events, the table outputs
int set_up_device(Batch& b, int64_t max_slice) {
    mhip_ctx* c = b.c;
    if (c->scratch("ca_jobs", sizeof(mhip_aln_job) * (size_t)b.nj, (void**)&b.d_jobs)) return -1;
    HIPCHK(hipMemcpyAsync(b.d_jobs, b.jobs.data(), sizeof(mhip_aln_job) * (size_t)b.nj, hipMemcpyHostToDevice, c->stream));
    for (int set = 0; set < std::min(2, b.nslices); ++set) {
        if (scratch_set(c, "ca_res", set, sizeof(mhip_cns_result) * (size_t)max_slice, (void**)&b.d_res[set])) return -1;
        if (scratch_set(c, "ca_ops", set, sizeof(uint32_t) * (size_t)b.row_words * (size_t)max_slice, (void**)&b.d_ops[set])) return -1;
    }
    b.res.resize((size_t)b.nj);
    HIPCHK(hipStreamCreateWithFlags(&b.copy_stream, hipStreamNonBlocking));
    for (int set = 0; set < 2; ++set) {
        HIPCHK(hipEventCreateWithFlags(&b.ev_built[set], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&b.ev_copied[set], hipEventDisableTiming));
    }
    if (b.TW > 0) {
        b.tab.reset((uint32_t*)result_alloc(sizeof(uint32_t) * (size_t)b.TW, b.threads)); b.ident.reset((uint8_t*)result_alloc((size_t)b.TW, b.threads));
        if (!b.tab || !b.ident) { mhip_set_error("out of memory (%lld table positions)", (long long)b.TW); return -1; }
    }
    if (const char* e = getenv("MECAT_CNS_STR_ESTIMATE")) b.est_scale = std::max(0.01, atof(e) / 100.0);
    return 0;
}

int align_slice(Batch& b, const Slice& sl, int set) {
    mhip_ctx* c = b.c;
    if (mhip_cns_align_candidates_dev(c, b.a.vol, b.a.vol, b.d_jobs + sl.j0, (int)sl.nj, b.error_rate, b.a.min_align_size, b.cap, b.d_res[set], b.d_ops[set])) return -1;
    HIPCHK(hipMemcpyAsync(b.res.data() + sl.j0, b.d_res[set], sizeof(mhip_cns_result) * (size_t)sl.nj, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// the sequential accept decisions, per template (host threads), and where the accepted alignments' strings go in the slice's buffer
void replay_slice(const Batch& b, Slice& sl) {
    const AcceptCall& a = b.a;
    const int nt = sl.t1 - sl.t0;
    sl.acc.assign((size_t)nt, std::vector<int32_t>()); sl.er.assign((size_t)(b.build_plan ? nt : 0), std::vector<int32_t>());
    parallel_for(nt, b.threads, [&](int64_t tl) {
        const int64_t t = sl.t0 + tl;
        if (a.tmpl_begin[t + 1] == a.tmpl_begin[t]) return;
        sl.acc[(size_t)tl] = a.input_type == 0 ? cns_replay_template(a.cands, a.tmpl_begin, b.res.data(), b.jfirst.data(), t, b.rules)
                                               : cns_replay_template_m4(a.cands, a.tmpl_begin, b.res.data(), b.jfirst.data(), t, b.m4);
        if (b.build_plan) {                                         // cns_vec.get_mapping_ranges + get_effective_ranges, :445-447 (tech 1: :509)
            std::vector<std::pair<int32_t, int32_t>> mr;
            for (const int32_t ji : sl.acc[(size_t)tl]) mr.emplace_back(b.res[(size_t)ji].soff, b.res[(size_t)ji].send);
            cns_effective_ranges(mr, b.read_size((int)t), a.tech, a.min_size, sl.er[(size_t)tl]);
        }
    });
    sl.afirst.assign((size_t)nt + 1, 0);
    for (int tl = 0; tl < nt; ++tl) sl.afirst[(size_t)tl + 1] = sl.afirst[(size_t)tl] + (int64_t)sl.acc[(size_t)tl].size();
    sl.items.resize((size_t)sl.afirst[(size_t)nt]);
    size_t off = 0;
    for (int tl = 0; tl < nt; ++tl)
        for (size_t k = 0; k < sl.acc[(size_t)tl].size(); ++k) {
            const int64_t ji = sl.acc[(size_t)tl][k];
            CnsStrItem& it = sl.items[(size_t)(sl.afirst[(size_t)tl] + (int64_t)k)];
            it.job = (int32_t)(ji - sl.j0); it.off = (unsigned long long)off;
            it.aln_size = b.res[(size_t)ji].last_col - b.res[(size_t)ji].first_col;          // O(ND) columns are matches or indels: normalising adds no columns
            off += 2 * ((size_t)it.aln_size + 1);
        }
    sl.sbytes = off;
}

// ---- the strings of an (aligned, replayed) slice: built on the device behind whatever the stream holds, copied on the second stream;
// the slice's tables (whole templates: a contiguous piece of the output) zeroed, tallied from the strings and finished behind them; its
// plan, pieces and consensus behind those.  strings_slice runs the steps; SliceWork is what one leaves for the next.
struct SliceWork {
    int set = 0, nt = 0;
    int64_t na = 0, tw0 = 0, tw = 0;       // accepted alignments; the slice's table words in the batch's
    size_t a0 = 0;                         // its first accepted record in Avec
    char* d_str = nullptr; uint32_t* d_tab = nullptr; uint8_t* d_id = nullptr;
    CnsPlanDev pd; CnsPiecesDev qd; CnsPoaDev od; CnsReadsDev rd; CnsTextDev td;
    PlanSlice* ps = nullptr;               // with a plan launched
};

// room for the slice's strings behind those of the slices before it
int reserve_strings(Batch& b, const Slice& sl, int k) {
    size_t want = b.S_used + sl.sbytes;
    if (want > b.S_cap && k + 1 < b.nslices)
        want = std::max(want, (size_t)((double)want / (double)sl.t1 * (double)b.a.num_templates * b.est_scale) + ((size_t)1 << 20));
    if (want <= b.S_cap) return 0;
    if (hipStreamSynchronize(b.copy_stream) != hipSuccess) { mhip_set_error("cns accept: copy stream failed"); return -1; }      // the copies into the old buffer have landed
    CnsBuf<char> nS(want >= ((size_t)64 << 20) ? strbuf_get(want, b.threads) : (char*)malloc(std::max<size_t>(want, 1)));
    if (!nS) { mhip_set_error("out of memory (%lld bytes of aligned strings)", (long long)want); return -1; }
    parallel_memcpy(nS.get(), b.S.get(), b.S_used, b.threads);
    b.S = std::move(nS); b.S_cap = want;
    return 0;
}

// the accepted records (what the caller gets beside the strings) and the table kernels' items
void build_records(Batch& b, const Slice& sl, const SliceWork& w, std::vector<CnsTabItem>& titems) {
    const AcceptCall& a = b.a;
    titems.resize((size_t)(b.build_tab ? w.na : 0));
    b.Avec.resize(w.a0 + (size_t)w.na);
    parallel_for(w.nt, b.threads, [&](int64_t tl) {
        const int64_t t = sl.t0 + tl;
        for (size_t kk = 0; kk < sl.acc[(size_t)tl].size(); ++kk) {
            const int64_t ji = sl.acc[(size_t)tl][kk], i = sl.afirst[(size_t)tl] + (int64_t)kk;
            const mhip_cns_result& r = b.res[(size_t)ji];
            const CnsStrItem& it = sl.items[(size_t)i];
            const mhip_ext_candidate& ec = a.cands[a.tmpl_begin[t] + (ji - b.jfirst[(size_t)t])];
            mhip_cns_accepted& o = b.Avec[w.a0 + (size_t)i];
            o.template_index = (int32_t)t; o.cand_index = a.tmpl_begin[t] + (ji - b.jfirst[(size_t)t]);
            o.qid = ec.qid; o.sid = ec.sid; o.qoff = r.qoff; o.qend = r.qend; o.soff = r.soff; o.send = r.send; o.aln_size = it.aln_size;
            o.str_offset = b.want_str ? (int64_t)(b.S_used + it.off) : -1;
            if (b.build_tab) {
                CnsTabItem& ti = titems[(size_t)i];
                ti.off = it.off; ti.tab = (unsigned long long)(b.TB[(size_t)t] - w.tw0); ti.aln_size = it.aln_size; ti.soff = r.soff;
                ti.tab_len = (int32_t)(b.TB[(size_t)t + 1] - b.TB[(size_t)t]); ti.pad = 0;
            }
        }
    });
}

int launch_strings(Batch& b, const Slice& sl, SliceWork& w) {
    mhip_ctx* c = b.c;
    CnsStrItem* d_items;
    if (scratch_set(c, "ca_str", w.set, sl.sbytes + 128, (void**)&w.d_str)) return -1;
    if (scratch_set(c, "ca_items", w.set, sizeof(CnsStrItem) * (size_t)w.na, (void**)&d_items)) return -1;
    HIPCHK(hipMemcpyAsync(d_items, b.hold_items[w.set].data(), sizeof(CnsStrItem) * (size_t)w.na, hipMemcpyHostToDevice, c->stream));
    return cns_strings_launch(c, b.a.vol, b.d_jobs + sl.j0, b.d_res[w.set], b.d_ops[w.set], b.row_words, d_items, (int)w.na, w.d_str);
}

int launch_tables(Batch& b, const Slice& sl, SliceWork& w) {
    mhip_ctx* c = b.c;
    std::vector<long long>& first = b.hold_first[w.set]; std::vector<int32_t>& voloff = b.hold_voloff[w.set];
    first.clear(); voloff.clear();
    for (int t = sl.t0; t < sl.t1; ++t)
        if (b.TB[(size_t)t + 1] > b.TB[(size_t)t]) {
            first.push_back((long long)(b.TB[(size_t)t] - w.tw0));
            voloff.push_back(b.a.vol->h_offs[(size_t)(b.a.cands[b.a.tmpl_begin[t]].sid - b.start_id)].offset);
        }
    const int ntm = (int)voloff.size();
    first.push_back((long long)w.tw);
    CnsTabItem* d_titems; long long* d_first; int32_t* d_voloff;
    if (scratch_set(c, "ca_tab", w.set, sizeof(uint32_t) * (size_t)w.tw, (void**)&w.d_tab)) return -1;
    if (scratch_set(c, "ca_ident", w.set, (size_t)w.tw, (void**)&w.d_id)) return -1;
    if (scratch_set(c, "ca_titems", w.set, sizeof(CnsTabItem) * (size_t)std::max<int64_t>(w.na, 1), (void**)&d_titems)) return -1;
    if (scratch_set(c, "ca_tfirst", w.set, sizeof(long long) * ((size_t)ntm + 1), (void**)&d_first)) return -1;
    if (scratch_set(c, "ca_tvoloff", w.set, sizeof(int32_t) * (size_t)ntm, (void**)&d_voloff)) return -1;
    if (w.na) HIPCHK(hipMemcpyAsync(d_titems, b.hold_titems[w.set].data(), sizeof(CnsTabItem) * (size_t)w.na, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_first, first.data(), sizeof(long long) * ((size_t)ntm + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_voloff, voloff.data(), sizeof(int32_t) * (size_t)ntm, hipMemcpyHostToDevice, c->stream));
    return cns_table_launch(c, b.a.vol, w.d_str, d_titems, (int)w.na, w.d_tab, w.d_id, (long long)w.tw, d_first, d_voloff, ntm, nullptr);
}

// host buffers for what a launch of the plan, the pieces or the consensus will copy out: `cap` elements and, with n >= 0, begin[n + 1]
bool slice_out_alloc(SliceOut& o, size_t elem, int64_t cap, int64_t n, int threads) {
    o.cap = cap;
    o.data.reset(result_alloc(elem * (size_t)cap, threads));
    if (n >= 0) o.begin.reset((int64_t*)result_alloc(sizeof(int64_t) * ((size_t)n + 1), threads));
    return o.data && (n < 0 || o.begin);
}

// the slice's plan, behind cns_table_finish on the same stream and in front of the copies; the windows' pieces behind cns_plan_emit (the
// slice's strings and plan are in place), their consensus behind cns_pieces_emit (the pieces stay where they are).  Each waits for the
// stream once: its counts size the host buffers
int launch_plan(Batch& b, const Slice& sl, SliceWork& w) {
    mhip_ctx* c = b.c; const int nt = w.nt;
    std::vector<long long> tbl((size_t)nt + 1), rbl((size_t)nt + 1, 0);
    std::vector<int32_t> erl;
    for (int tl = 0; tl <= nt; ++tl) tbl[(size_t)tl] = (long long)(b.TB[(size_t)(sl.t0 + tl)] - w.tw0);
    for (int tl = 0; tl < nt; ++tl) {
        erl.insert(erl.end(), sl.er[(size_t)tl].begin(), sl.er[(size_t)tl].end());
        rbl[(size_t)tl + 1] = (long long)(erl.size() / 2);
        b.ERB[(size_t)(sl.t0 + tl) + 1] = (int64_t)(sl.er[(size_t)tl].size() / 2);
    }
    b.ER.insert(b.ER.end(), erl.begin(), erl.end());
    if (cns_plan_launch(c, w.set, w.d_tab, w.d_id, nt, sl.t0, tbl.data(), erl.data(), rbl.data(), b.a.min_cov, b.min_run, b.seg_total, b.win_total, b.SB.data() + sl.t0, &w.pd)) return -1;
    b.tk[LAP_PLAN_WAIT] += w.pd.wait_s;
    const CnsPlanDev& pd = w.pd;
    b.plan.emplace_back();
    PlanSlice& ps = b.plan.back();
    w.ps = &ps;
    ps.seg.count = pd.nseg; ps.win.count = pd.nwin; ps.pc.n = ps.cn.n = pd.nwin;               // (the windows own nothing until pieces and consensus have run)
    const bool room = !b.want_plan || (slice_out_alloc(ps.seg, sizeof(mhip_cns_segment), pd.nseg, -1, b.threads) && slice_out_alloc(ps.win, sizeof(mhip_cns_window), pd.nwin, -1, b.threads));
    if (!room) { mhip_set_error("out of memory (%lld windows)", (long long)pd.nwin); return -1; }
    if (b.build_pieces && pd.nwin > 0 && w.na > 0) {
        std::vector<CnsPieceItem> pitems((size_t)w.na);
        std::vector<long long> afl(sl.afirst.begin(), sl.afirst.end());
        parallel_for(nt, b.threads, [&](int64_t tl) {
            for (int64_t i = sl.afirst[(size_t)tl]; i < sl.afirst[(size_t)tl + 1]; ++i) {
                const mhip_cns_accepted& o = b.Avec[w.a0 + (size_t)i];
                CnsPieceItem& it = pitems[(size_t)i];
                it.off = b.hold_items[w.set][(size_t)i].off; it.aln_size = o.aln_size; it.soff = o.soff; it.send = o.send; it.tl = (int32_t)tl;
            }
        });
        if (cns_pieces_launch(c, w.set, w.d_str, pitems.data(), w.na, (long long)w.a0, nt, sl.t0, afl.data(), tbl.data(), pd.d_seg, pd.nseg, pd.d_segb, b.seg_total, b.win_total, pd.d_win,
                              pd.nwin, &w.qd)) return -1;
        b.tk[LAP_PLAN_WAIT] += w.qd.wait_s;
        if (b.want_pieces && !slice_out_alloc(ps.pc, sizeof(mhip_cns_piece), w.qd.cap, pd.nwin, b.threads)) { mhip_set_error("out of memory (%lld pieces)", (long long)w.qd.cap); return -1; }
        if (b.build_poa) {
            if (cns_poa_launch(c, w.set, w.d_str, w.qd, w.na, (long long)w.a0, pd.d_win, pd.nwin, &w.od)) return -1;
            b.tk[LAP_PLAN_WAIT] += w.od.wait_s; b.poa_large += w.od.nlarge; b.poa_chunks += w.od.nchunks;
            if (b.want_poa && !slice_out_alloc(ps.cn, 1, w.od.cap, pd.nwin, b.threads)) { mhip_set_error("out of memory (%lld bytes of consensus)", (long long)w.od.cap); return -1; }
        }
    }
    if (b.build_reads && pd.nseg > 0) {           // (a segment without a window is a read of its anchors' letters)
        std::vector<int32_t> rid((size_t)nt, 0);
        for (int tl = 0; tl < nt; ++tl)
            if (b.a.tmpl_begin[sl.t0 + tl + 1] > b.a.tmpl_begin[sl.t0 + tl]) rid[(size_t)tl] = b.a.cands[b.a.tmpl_begin[sl.t0 + tl]].sid;
        if (cns_reads_launch(c, w.set, w.d_tab, w.d_id, nt, sl.t0, tbl.data(), rid.data(), pd.d_seg, pd.nseg, pd.d_segb, b.seg_total, b.win_total, pd.d_win, pd.nwin, w.od.d_cns,
                             w.od.d_cb, w.od.cap, b.a.min_size, &w.rd)) return -1;
        b.tk[LAP_PLAN_WAIT] += w.rd.wait_s; b.reads_wait += w.rd.wait_s;
        ps.t0 = sl.t0; ps.nt = nt;
        if (b.want_reads) {
            ps.rd.count = w.rd.nreads; ps.sq.count = w.rd.seq_bytes;
            ps.tbegin.reset((int64_t*)result_alloc(sizeof(int64_t) * ((size_t)nt + 1), b.threads));
            if (!slice_out_alloc(ps.rd, sizeof(mhip_cns_read), w.rd.nreads, -1, b.threads) || !slice_out_alloc(ps.sq, 1, w.rd.seq_bytes, -1, b.threads) || !ps.tbegin) {
                mhip_set_error("out of memory (%lld bytes of corrected reads)", (long long)w.rd.seq_bytes); return -1;
            }
        }
        if (b.want_text && w.rd.nreads > 0) {     // behind cns_reads_letters, in front of the copies
            if (cns_text_launch(c, w.set, w.rd.d_reads, w.rd.nreads, w.rd.d_seq, w.rd.seq_bytes, &w.td)) return -1;
            b.tk[LAP_PLAN_WAIT] += w.td.wait_s; b.text_wait += w.td.wait_s;
            ps.tx.count = w.td.bytes;
            if (!slice_out_alloc(ps.tx, 1, w.td.bytes, -1, b.threads)) { mhip_set_error("out of memory (%lld bytes of text)", (long long)w.td.bytes); return -1; }
        }
    }
    b.seg_total += pd.nseg; b.win_total += pd.nwin;
    return 0;
}

// everything the slice's launches left goes to the host on the copy stream, behind ev_built; ev_copied tells when the set is free again
int enqueue_copies(Batch& b, const Slice& sl, const SliceWork& w) {
    const int set = w.set; hipStream_t cs = b.copy_stream;
    HIPCHK(hipEventRecord(b.ev_built[set], b.c->stream));
    HIPCHK(hipStreamWaitEvent(cs, b.ev_built[set], 0));
    if (b.want_str && w.na) {
        HIPCHK(hipMemcpyAsync(b.S.get() + b.S_used, w.d_str, sl.sbytes, hipMemcpyDeviceToHost, cs));
        b.S_used += sl.sbytes;
    }
    const CnsPlanDev& pd = w.pd;
    if (pd.nseg && b.want_plan) HIPCHK(hipMemcpyAsync(w.ps->seg.data.get(), pd.d_seg, sizeof(mhip_cns_segment) * (size_t)pd.nseg, hipMemcpyDeviceToHost, cs));
    if (pd.nwin && b.want_plan) HIPCHK(hipMemcpyAsync(w.ps->win.data.get(), pd.d_win, sizeof(mhip_cns_window) * (size_t)pd.nwin, hipMemcpyDeviceToHost, cs));
    if (pd.d_bad) HIPCHK(hipMemcpyAsync(&w.ps->win.bad, pd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, cs));      // (b.plan: reserved, nothing moves)
    if (w.qd.d_pb) {                          // (the slots the bound allows; how many hold records is begin[nwin], read at the hand-over)
        SliceOut& pc = w.ps->pc;
        if (b.want_pieces) {
            if (w.qd.cap) HIPCHK(hipMemcpyAsync(pc.data.get(), w.qd.d_pieces, sizeof(mhip_cns_piece) * (size_t)w.qd.cap, hipMemcpyDeviceToHost, cs));
            HIPCHK(hipMemcpyAsync(pc.begin.get(), w.qd.d_pb, sizeof(int64_t) * ((size_t)pd.nwin + 1), hipMemcpyDeviceToHost, cs));
        }
        HIPCHK(hipMemcpyAsync(&pc.bad, w.qd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, cs));
    }
    if (w.od.d_cb) {                          // (the bytes the bound allows; how many hold strings is begin[nwin], read at the hand-over)
        SliceOut& cn = w.ps->cn;
        if (b.want_poa) {
            if (w.od.cap) HIPCHK(hipMemcpyAsync(cn.data.get(), w.od.d_cns, (size_t)w.od.cap, hipMemcpyDeviceToHost, cs));
            HIPCHK(hipMemcpyAsync(cn.begin.get(), w.od.d_cb, sizeof(int64_t) * ((size_t)pd.nwin + 1), hipMemcpyDeviceToHost, cs));
        }
        HIPCHK(hipMemcpyAsync(&cn.bad, w.od.d_bad, sizeof(long long), hipMemcpyDeviceToHost, cs));
    }
    if (w.rd.d_bad) {                         // (exact sizes: cns_reads_launch has waited for the totals)
        PlanSlice& ps = *w.ps;
        if (b.want_reads) {
            if (w.rd.nreads) HIPCHK(hipMemcpyAsync(ps.rd.data.get(), w.rd.d_reads, sizeof(mhip_cns_read) * (size_t)w.rd.nreads, hipMemcpyDeviceToHost, cs));
            if (w.rd.seq_bytes) HIPCHK(hipMemcpyAsync(ps.sq.data.get(), w.rd.d_seq, (size_t)w.rd.seq_bytes, hipMemcpyDeviceToHost, cs));
            HIPCHK(hipMemcpyAsync(ps.tbegin.get(), w.rd.d_tbegin, sizeof(int64_t) * ((size_t)w.nt + 1), hipMemcpyDeviceToHost, cs));
        }
        HIPCHK(hipMemcpyAsync(&ps.rd.bad, w.rd.d_bad, sizeof(long long), hipMemcpyDeviceToHost, cs));
    }
    if (w.td.d_bad) {                         // (exact size: cns_text_launch has waited for the total)
        HIPCHK(hipMemcpyAsync(w.ps->tx.data.get(), w.td.d_text, (size_t)w.td.bytes, hipMemcpyDeviceToHost, cs));
        HIPCHK(hipMemcpyAsync(&w.ps->tx.bad, w.td.d_bad, sizeof(long long), hipMemcpyDeviceToHost, cs));
    }
    if (w.tw && b.want_tab) {
        HIPCHK(hipMemcpyAsync(b.tab.get() + w.tw0, w.d_tab, sizeof(uint32_t) * (size_t)w.tw, hipMemcpyDeviceToHost, cs));
        HIPCHK(hipMemcpyAsync(b.ident.get() + w.tw0, w.d_id, (size_t)w.tw, hipMemcpyDeviceToHost, cs));
    }
    HIPCHK(hipEventRecord(b.ev_copied[set], cs));
    return 0;
}

int strings_slice(Batch& b, Slice& sl, int set, int k) {
    SliceWork w;
    w.set = set; w.nt = sl.t1 - sl.t0; w.na = (int64_t)sl.items.size();
    w.tw0 = b.build_tab ? b.TB[(size_t)sl.t0] : 0; w.tw = b.build_tab ? b.TB[(size_t)sl.t1] - w.tw0 : 0; w.a0 = b.Avec.size();
    if (b.build_plan) for (int t = sl.t0; t <= sl.t1; ++t) b.SB[(size_t)t] = b.seg_total;      // (what a slice without a table leaves)
    if (w.na == 0 && w.tw == 0) return 0;
    if (b.want_str && w.na && reserve_strings(b, sl, k)) return -1;
    std::vector<CnsTabItem> titems;
    build_records(b, sl, w, titems);
    if (k >= 2) HIPCHK(hipEventSynchronize(b.ev_copied[set]));      // the copies out of this set's buffers two slices ago (the string buffer may move)
    // (that slice's host arrays are done with now: this slice's take their place)
    b.hold_items[set].swap(sl.items); b.hold_titems[set].swap(titems);
    if (w.na && launch_strings(b, sl, w)) return -1;
    if (w.tw && launch_tables(b, sl, w)) return -1;
    if (b.build_plan && w.tw && launch_plan(b, sl, w)) return -1;
    return enqueue_copies(b, sl, w);
}

template <typename T> CnsBuf<T> copy_of(const T* src, size_t n) {
    CnsBuf<T> p((T*)malloc(std::max<size_t>(sizeof(T) * n, 1)));
    if (p && n) memcpy(p.get(), src, sizeof(T) * n);
    return p;
}

struct PlanResult { CnsBuf<void> seg, win, pc, cn, reads, seq, text; CnsBuf<int64_t> seg_begin, erange_begin, piece_begin, cns_begin, read_begin; CnsBuf<int32_t> eranges; };

// concat_slices over one member of the plan's slices; its refusals in the output's own words (counts: two %lld, no_memory: one)
struct ConcatTexts { const char *bad, *counts, *no_memory; };
int concat(Batch& b, SliceOut PlanSlice::*member, size_t elem, CnsBuf<void>* data, CnsBuf<int64_t>* begin, const ConcatTexts& tx) {
    std::vector<SliceOut*> parts;
    for (PlanSlice& p : b.plan) parts.push_back(&(p.*member));
    int64_t total = 0, counts[2] = {0, 0};
    const int rc = concat_slices(parts, elem, b.threads, data, begin, &total, counts);
    if (rc == CONCAT_BAD_FLAG) mhip_set_error("%s", tx.bad);
    if (rc == CONCAT_COUNTS) mhip_set_error(tx.counts, (long long)counts[0], (long long)counts[1]);
    if (rc == CONCAT_NO_MEMORY) mhip_set_error(tx.no_memory, (long long)total);
    return rc ? -1 : 0;
}

// the slices' reads behind one another: the records are final except seq_begin, which gets its batch-wide base here; a template's
// first record from the slices' tbegin[]
int put_reads_together(Batch& b, PlanResult& r) {
    const char* reads_bad = "cns reads: an index left its array, or the letters written are not the letters counted";
    const size_t n1 = (size_t)b.a.num_templates + 1;
    if (concat(b, &PlanSlice::rd, sizeof(mhip_cns_read), &r.reads, nullptr, {reads_bad, "", "out of memory (%lld reads)"})) return -1;
    if (concat(b, &PlanSlice::sq, 1, &r.seq, nullptr, {reads_bad, "", "out of memory (%lld bytes of corrected reads)"})) return -1;
    r.read_begin.reset((int64_t*)calloc(n1, sizeof(int64_t)));
    if (!r.read_begin) { mhip_set_error("out of memory"); return -1; }
    mhip_cns_read* R = (mhip_cns_read*)r.reads.get();
    int64_t* RB = r.read_begin.get();
    int64_t rbase = 0, sbase = 0;
    for (const PlanSlice& p : b.plan) {
        if (!p.tbegin) continue;
        const int64_t* tb = p.tbegin.get();
        bool ok = tb[0] == 0 && tb[p.nt] == p.rd.count;
        for (int tl = 0; tl < p.nt && ok; ++tl) {
            ok = tb[tl + 1] >= tb[tl];
            RB[(size_t)(p.t0 + tl) + 1] = tb[tl + 1] - tb[tl];          // counts -> first record of every template, below
        }
        for (int64_t i = 0; i < p.rd.count && ok; ++i) {
            mhip_cns_read& x = R[rbase + i];
            ok = x.size > 0 && x.seq_begin >= 0 && x.seq_begin + x.size <= p.sq.count;
            x.seq_begin += sbase;
        }
        if (!ok) { mhip_set_error("%s", reads_bad); return -1; }
        rbase += p.rd.count; sbase += p.sq.count;
    }
    for (size_t t = 0; t + 1 < n1; ++t) RB[t + 1] += RB[t];
    b.reads_total = rbase; b.seq_total = sbase;
    return 0;
}

// the slices' parts of the plan put together (after the last copy has landed)
int put_plan_together(Batch& b, PlanResult& r) {
    const char* pieces_bad = "cns pieces: an index left its array, or the pieces written are not the pieces counted";
    const char* poa_bad = "cns poa: a window's graph left its workspace bound, or a piece leaves its backbone";
    const size_t n1 = (size_t)b.a.num_templates + 1;
    if (b.want_plan) {
        if (concat(b, &PlanSlice::win, sizeof(mhip_cns_window), &r.win, nullptr, {"cns plan: the windows written are not the windows counted", "", "out of memory"})) return -1;
        if (concat(b, &PlanSlice::seg, sizeof(mhip_cns_segment), &r.seg, nullptr, {"", "", "out of memory"})) return -1;
    }
    for (const PlanSlice& p : b.plan) {        // (the flags come with the stages that were built, copied or not)
        if (p.win.bad) { mhip_set_error("cns plan: the windows written are not the windows counted"); return -1; }
        if (p.cn.bad) { mhip_set_error("%s", poa_bad); return -1; }
    }
    for (const PlanSlice& p : b.plan)          // (the flag comes with POA alone as well)
        if (p.pc.bad) { mhip_set_error("%s", pieces_bad); return -1; }
    if (b.want_pieces && concat(b, &PlanSlice::pc, sizeof(mhip_cns_piece), &r.pc, &r.piece_begin,
                                {pieces_bad, "cns pieces: inconsistent counts (%lld pieces in %lld slots)", "out of memory (%lld pieces)"})) return -1;
    if (b.want_poa && concat(b, &PlanSlice::cn, 1, &r.cn, &r.cns_begin, {poa_bad,
                                                                          "cns poa: inconsistent counts (%lld bytes in %lld)", "out of memory (%lld bytes of consensus)"})) return -1;
    if (b.want_reads && put_reads_together(b, r)) return -1;
    if (b.want_text) {                         // (template order, whole templates per slice: the slices' texts as they are, one behind the other)
        for (const PlanSlice& p : b.plan)
            if (p.rd.bad) { mhip_set_error("cns reads: an index left its array, or the letters written are not the letters counted"); return -1; }
        if (concat(b, &PlanSlice::tx, 1, &r.text, nullptr, {"cns text: a record leaves the letters or holds a negative number, or the bytes written are not the bytes counted", "",
                                                             "out of memory (%lld bytes of text)"})) return -1;
        for (const PlanSlice& p : b.plan) b.text_total += p.tx.count;
    }
    if (!b.want_plan) return 0;
    for (size_t t = 0; t + 1 < n1; ++t) b.ERB[t + 1] += b.ERB[t];          // counts -> first range of every template
    r.seg_begin = copy_of(b.SB.data(), n1); r.erange_begin = copy_of(b.ERB.data(), n1); r.eranges = copy_of(b.ER.data(), b.ER.size());
    if (!r.seg_begin || !r.erange_begin || !r.eranges) { mhip_set_error("out of memory"); return -1; }
    return 0;
}

// Every output goes to the caller, or none: the buffers change hands once nothing can fail any more (after the last copy has landed)
int hand_over(Batch& b) {
    const AcceptCall& a = b.a;
    const int64_t na = (int64_t)b.Avec.size(), sbytes = (int64_t)b.S_used;
    CnsBuf<mhip_cns_accepted> A; CnsBuf<int64_t> table_begin; PlanResult r;
    if (na && !(A = copy_of(b.Avec.data(), (size_t)na))) { mhip_set_error("out of memory"); return -1; }
    if (b.want_tab && !(table_begin = copy_of(b.TB.data(), (size_t)a.num_templates + 1))) { mhip_set_error("out of memory"); return -1; }
    const double t_put = now();
    const int plan_rc = b.build_plan ? put_plan_together(b, r) : 0;
    b.tk[LAP_PUT] += now() - t_put;
    if (plan_rc) return -1;
    b.lap(LAP_LAST_COPIES);
    if (na && getenv("MECAT_CNS_TIMES")) {
        const double* tk = b.tk;
        fprintf(stderr, "[cns_accept] %d templates, %lld jobs in %d slices, %lld accepted, %.2f GB of strings: sort + checks %.3f s, jobs %.3f, re-alignment on the "
                        "device %.3f, accept replay beyond it %.3f, strings launched %.3f, last copies %.3f\n", a.num_templates, (long long)b.nj, b.nslices, (long long)na,
                (double)sbytes / 1e9, tk[LAP_SORT], tk[LAP_JOBS], tk[LAP_ALIGN], tk[LAP_REPLAY], tk[LAP_STRINGS], tk[LAP_LAST_COPIES]);
        if (b.want_pieces) fprintf(stderr, "[cns_accept] pieces: %lld pieces (the waits for their bound are counted with the plan's)\n", (long long)r.piece_begin.get()[b.win_total]);
        if (b.want_poa)
            fprintf(stderr, "[cns_accept] poa: %lld bytes of consensus, %lld windows in cns_poa_large (%lld launches); the waits for the bounds are counted with the plan's\n",
                    (long long)r.cns_begin.get()[b.win_total], b.poa_large, b.poa_chunks);
        if (b.want_reads)
            fprintf(stderr, "[cns_accept] reads: %lld records, %lld bytes of corrected reads: waited for the totals %.3f s (counted with the plan's waits)\n", (long long)b.reads_total,
                    (long long)b.seq_total, b.reads_wait);
        if (b.want_text)
            fprintf(stderr, "[cns_accept] text: %lld bytes: waited for the totals %.3f s (counted with the plan's waits)\n", (long long)b.text_total, b.text_wait);
        if (b.build_plan)
            fprintf(stderr, "[cns_accept] plan: %lld segments, %lld windows: waited for the counts %.3f s (within strings launched), slices' pieces put together %.3f (within last copies)\n",
                    (long long)b.seg_total, (long long)b.win_total, tk[LAP_PLAN_WAIT], tk[LAP_PUT]);
    }
    if (na) { *a.accepted = A.release(); *a.count = na; *a.strings = b.S.release(); *a.strings_bytes = sbytes; }
    if (b.want_tab) { *a.table = (mhip_cns_table_item*)b.tab.release(); *a.ident = b.ident.release(); *a.table_begin = table_begin.release(); }
    if (b.want_plan) {
        *a.segments = (mhip_cns_segment*)r.seg.release(); *a.seg_begin = r.seg_begin.release(); *a.windows = (mhip_cns_window*)r.win.release(); *a.n_windows = b.win_total;
        *a.eranges = r.eranges.release(); *a.erange_begin = r.erange_begin.release();
    }
    if (b.want_pieces) { *a.pieces = (mhip_cns_piece*)r.pc.release(); *a.piece_begin = r.piece_begin.release(); }
    if (b.want_poa) { *a.cns = (char*)r.cn.release(); *a.cns_begin = r.cns_begin.release(); }
    if (b.want_reads) { *a.reads = (mhip_cns_read*)r.reads.release(); *a.read_begin = r.read_begin.release(); *a.seq = (char*)r.seq.release(); *a.seq_bytes = b.seq_total; }
    if (b.want_text) { *a.text = (char*)r.text.release(); *a.text_bytes = b.text_total; }
    return 0;
}

int run(const AcceptCall& a, int allowed) {
    if (validate(a, allowed)) return -1;
    HIPCHK(hipSetDevice(a.c->device));
    const int T = a.num_templates;
    if (T <= 0) return 0;
    Batch b(a);
    if (sort_and_check(b)) return -1;
    if (b.build_tab) {
        b.TB.assign((size_t)T + 1, 0);
        for (int t = 0; t < T; ++t) b.TB[(size_t)t + 1] = b.TB[(size_t)t] + (a.tmpl_begin[t + 1] > a.tmpl_begin[t] ? (int64_t)b.read_size(t) : 0);
    }
    b.TW = b.want_tab ? b.TB[(size_t)T] : 0;
    if (b.build_plan) { b.SB.assign((size_t)T + 1, 0); b.ERB.assign((size_t)T + 1, 0); }
    b.lap(LAP_SORT);
    b.jfirst.assign((size_t)T + 1, 0);
    const int64_t max_jobs = a.input_type == 0 ? b.rules.max_ext : b.m4.max_added;
    for (int t = 0; t < T; ++t) b.jfirst[(size_t)t + 1] = b.jfirst[(size_t)t] + std::min<int64_t>(max_jobs, a.tmpl_begin[t + 1] - a.tmpl_begin[t]);
    b.nj = b.jfirst[(size_t)T];
    if (a.jobs) *a.jobs = b.nj;
    if (b.nj == 0) return hand_over(b);
    if (b.nj > 0x7fffffffLL) { mhip_set_error("cns accept: too many jobs in one batch"); return -1; }
    make_jobs(b);
    std::vector<Slice> slices = cut_slices(b);
    b.nslices = (int)slices.size(); b.plan.reserve(slices.size());
    int64_t max_slice = 0;
    for (const Slice& sl : slices) max_slice = std::max(max_slice, sl.nj);
    if (set_up_device(b, max_slice)) return -1;
    b.lap(LAP_JOBS);
    if (slices[0].nj > 0 && align_slice(b, slices[0], 0)) return -1;
    b.lap(LAP_ALIGN);
    for (int k = 0; k < b.nslices; ++k) {
        Slice& sl = slices[(size_t)k];
        std::thread rp([&]() { replay_slice(b, sl); });
        const int rc = k + 1 < b.nslices && slices[(size_t)k + 1].nj > 0 ? align_slice(b, slices[(size_t)k + 1], (k + 1) & 1) : 0;
        b.lap(LAP_ALIGN);
        rp.join();
        b.lap(LAP_REPLAY);
        if (rc || strings_slice(b, sl, k & 1, k)) return -1;
        sl.acc.clear(); sl.acc.shrink_to_fit(); sl.items.clear(); sl.items.shrink_to_fit();
        b.lap(LAP_STRINGS);
    }
    HIPCHK(hipStreamSynchronize(b.copy_stream));
    return hand_over(b);
}

}  // namespace

extern "C" {

int mhip_cns_accept_templates(mhip_ctx* c, const mhip_volume* vol, const uint8_t* /*host_pac: not read any more (the strings are built on the device)*/, mhip_ext_candidate* cands,
                              const int64_t* tmpl_begin, int num_templates, int tech, int min_align_size, double min_mapping_ratio, int num_threads, mhip_cns_accepted** out_accepted,
                              int64_t* out_count, char** out_strings, int64_t* out_strings_bytes, int64_t* out_jobs) {
    return run({c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, WANT_STR, 0, 0, out_accepted, out_count, out_strings, out_strings_bytes, out_jobs}, WANT_STR);
}

int mhip_cns_accept_templates_ex(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, int tech, int min_align_size,
                                 double min_mapping_ratio, int num_threads, int want, mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings, int64_t* out_strings_bytes,
                                 int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident, int64_t** out_table_begin) {
    return run({c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, want, 0, 0, out_accepted, out_count, out_strings, out_strings_bytes, out_jobs,
                out_table, out_ident, out_table_begin}, WANT_STR | WANT_TAB);
}

int mhip_cns_accept_templates_plan(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, int tech, int min_align_size,
                                   double min_mapping_ratio, int num_threads, int want, int min_cov, int min_size, mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings,
                                   int64_t* out_strings_bytes, int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident, int64_t** out_table_begin,
                                   mhip_cns_segment** out_segments, int64_t** out_seg_begin, mhip_cns_window** out_windows, int64_t* out_n_windows, int32_t** out_eranges, int64_t** out_erange_begin) {
    return run({c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, want, min_cov, min_size, out_accepted, out_count, out_strings, out_strings_bytes,
                out_jobs, out_table, out_ident, out_table_begin, out_segments, out_seg_begin, out_windows, out_n_windows, out_eranges, out_erange_begin}, WANT_STR | WANT_TAB | WANT_PLAN);
}

int mhip_cns_accept_templates_pieces(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, int tech, int min_align_size,
                                     double min_mapping_ratio, int num_threads, int want, int min_cov, int min_size, mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings,
                                     int64_t* out_strings_bytes, int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident, int64_t** out_table_begin,
                                     mhip_cns_segment** out_segments, int64_t** out_seg_begin, mhip_cns_window** out_windows, int64_t* out_n_windows, int32_t** out_eranges,
                                     int64_t** out_erange_begin, mhip_cns_piece** out_pieces, int64_t** out_piece_begin) {
    return run({c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, want, min_cov, min_size, out_accepted, out_count, out_strings, out_strings_bytes,
                out_jobs, out_table, out_ident, out_table_begin, out_segments, out_seg_begin, out_windows, out_n_windows, out_eranges, out_erange_begin, out_pieces, out_piece_begin}, WANT_STR | WANT_TAB | WANT_PLAN | WANT_PIECES);
}

int mhip_cns_accept_templates_poa(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, int tech, int min_align_size,
                                  double min_mapping_ratio, int num_threads, int want, int min_cov, int min_size, mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings,
                                  int64_t* out_strings_bytes, int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident, int64_t** out_table_begin,
                                  mhip_cns_segment** out_segments, int64_t** out_seg_begin, mhip_cns_window** out_windows, int64_t* out_n_windows, int32_t** out_eranges,
                                  int64_t** out_erange_begin, mhip_cns_piece** out_pieces, int64_t** out_piece_begin, char** out_cns, int64_t** out_cns_begin) {
    return run({c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, want, min_cov, min_size, out_accepted, out_count, out_strings, out_strings_bytes,
                out_jobs, out_table, out_ident, out_table_begin, out_segments, out_seg_begin, out_windows, out_n_windows, out_eranges, out_erange_begin, out_pieces, out_piece_begin, out_cns,
                out_cns_begin}, WANT_STR | WANT_TAB | WANT_PLAN | WANT_PIECES | WANT_POA);
}

int mhip_cns_accept_templates_reads(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, int tech, int min_align_size,
                                    double min_mapping_ratio, int num_threads, int want, int min_cov, int min_size, mhip_cns_accepted** out_accepted, int64_t* out_count, char** out_strings,
                                    int64_t* out_strings_bytes, int64_t* out_jobs, mhip_cns_table_item** out_table, uint8_t** out_ident, int64_t** out_table_begin,
                                    mhip_cns_segment** out_segments, int64_t** out_seg_begin, mhip_cns_window** out_windows, int64_t* out_n_windows, int32_t** out_eranges,
                                    int64_t** out_erange_begin, mhip_cns_piece** out_pieces, int64_t** out_piece_begin, char** out_cns, int64_t** out_cns_begin,
                                    mhip_cns_read** out_reads, int64_t** out_read_begin, char** out_seq, int64_t* out_seq_bytes) {
    return run({c, vol, cands, tmpl_begin, num_templates, tech, min_align_size, min_mapping_ratio, num_threads, want, min_cov, min_size, out_accepted, out_count, out_strings, out_strings_bytes,
                out_jobs, out_table, out_ident, out_table_begin, out_segments, out_seg_begin, out_windows, out_n_windows, out_eranges, out_erange_begin, out_pieces, out_piece_begin, out_cns,
                out_cns_begin, out_reads, out_read_begin, out_seq, out_seq_bytes}, WANT_STR | WANT_TAB | WANT_PLAN | WANT_PIECES | WANT_POA | WANT_READS);
}

int mhip_cns_correct_templates(mhip_ctx* c, const mhip_volume* vol, mhip_ext_candidate* cands, const int64_t* tmpl_begin, int num_templates, const mhip_cns_opts* o,
                               mhip_cns_outputs* out) {
    if (!o || !out) { mhip_set_error("cns accept: the options or the outputs are NULL"); return -1; }
    *out = mhip_cns_outputs();
    AcceptCall a{c, vol, cands, tmpl_begin, num_templates, o->tech, o->min_align_size, o->min_mapping_ratio, o->num_threads, o->want, o->min_cov, o->min_size,
                 &out->accepted, &out->count, &out->strings, &out->strings_bytes, &out->jobs, &out->table, &out->ident, &out->table_begin, &out->segments, &out->seg_begin,
                 &out->windows, &out->n_windows, &out->eranges, &out->erange_begin, &out->pieces, &out->piece_begin, &out->cns, &out->cns_begin, &out->reads, &out->read_begin,
                 &out->seq, &out->seq_bytes};
    a.input_type = o->input_type; a.text = &out->text; a.text_bytes = &out->text_bytes;
    return run(a, WANT_STR | WANT_TAB | WANT_PLAN | WANT_PIECES | WANT_POA | WANT_READS | WANT_TEXT);
}

void mhip_cns_outputs_free(mhip_cns_outputs* out) {
    if (!out) return;
    void* const p[] = {out->accepted, out->strings, out->table, out->ident, out->table_begin, out->segments, out->seg_begin, out->windows, out->eranges, out->erange_begin,
                       out->pieces, out->piece_begin, out->cns, out->cns_begin, out->reads, out->read_begin, out->seq, out->text};
    for (void* x : p) if (x) mhip_cns_free(x);
    *out = mhip_cns_outputs();
}

}  // extern "C"
