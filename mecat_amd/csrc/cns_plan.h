// cns_plan.h — mecat2cns' consensus plan (segments and POA windows) from the consensus tables on the device (cns_plan.hip), used by
// cns_accept.hip behind the table kernels of a slice
#pragma once
#include "common.h"

struct CnsPlanDev {
    const mhip_cns_segment* d_seg = nullptr;      // [nseg] final records (global template, segment and window numbers)
    const mhip_cns_window* d_win = nullptr;       // [nwin]
    const long long* d_segb = nullptr;            // [nt + 1] seg_begin on the device (what cns_pieces.hip finds a template's windows with)
    const long long* d_bad = nullptr;             // nonzero once cns_plan_emit has run: it did not write the windows that were counted (NULL: nothing ran)
    long long nseg = 0, nwin = 0;
    double wait_s = 0;                            // host seconds spent in the wait for the counts
};

// The plan of `nt` templates whose tables lie in d_table / d_ident (template k: words [tb[k], tb[k + 1]), tb[] relative to d_table) with
// effective ranges er[2 * rb[k] .. 2 * rb[k + 1]) (pairs, template coordinates, clamped to the template on the device).  tb, er, rb are
// HOST arrays.  Everything runs on c->stream behind what the stream holds; the function WAITS for the stream once (the number of
// windows decides the size of their buffer) and returns with cns_plan_emit launched.  `set` (0 / 1) picks the scratch buffers: the
// arrays behind `out` stay valid until the next call with the same set.  Records come out final: template_index = t_index0 + k,
// segment numbers from seg_base, window numbers from win_base; seg_begin[0 .. nt] (host) = seg_base + segments of the templates before k.
int cns_plan_launch(mhip_ctx* c, int set, const uint32_t* d_table, const uint8_t* d_ident, int nt, int t_index0, const long long* tb, const int32_t* er,
                    const long long* rb, int min_cov, int min_run, long long seg_base, long long win_base, int64_t* seg_begin, CnsPlanDev* out);
