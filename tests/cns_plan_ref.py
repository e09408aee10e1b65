"""Restatement, loop by loop, of what mecat2cns decides from a template's consensus table alone (mecat2cns/mecat_correction.cpp):

    effective_ranges   get_effective_ranges, :118-153 (called at :445-447 for PacBio; nanopore and the m4 variants take (0, read_size),
                       :509 / :357)
    segments           the coverage runs of consensus_worker, :203-239
    windows            the anchor walk of meap_consensus_one_segment, :81-108: which (sb, se) it hands to meap_cns_one_indel and with
                       which min_cov (:103)

Plain Python over lists, in the reference's own order of steps; checker of mhip_cns_accept_templates_plan / mhip_debug_cns_plan
(test_gpu_cns_plan.py) and held against hand-computed plans in test_cns_plan_ref_cpu.py.  No compiled-reference harness exposes these
decisions yet, so the plan is pinned through reference-recorded INPUTS (the tables and ident bytes of tests/golden/cns_table.npz, the
coordinates of cns_accept.npz), this restatement and hand-computed cases."""
import numpy as np

FMAT, FDEL, FINS, UNDS = 1, 2, 4, 8
SEGMENT_DTYPE = np.dtype([("template_index", np.int32), ("beg", np.int32), ("end", np.int32), ("n_anchors", np.int32), ("win_begin", np.int64),
                          ("win_end", np.int64)])
WINDOW_DTYPE = np.dtype([("sb", np.int32), ("se", np.int32), ("cov", np.int32), ("segment", np.int32)])
DEFAULTS = {0: (4, 5000), 1: (6, 2000)}          # tech -> (min_cov, min_size): mecat2cns' options for PacBio / nanopore


def effective_ranges(mranges, read_size, tech, min_size):
    """mranges: (start, end) of the accepted alignments in accept order -> list of (start, end)"""
    if read_size <= 0:                    # a template without candidates: the reference never gets to it
        return []
    if tech != 0:
        return [(0, read_size)]           # :509
    mranges = [(int(a), int(b)) for a, b in mranges]
    eranges = []
    if len(mranges) == 0:                 # :122
        return eranges
    for start, end in mranges:            # :124-129
        if start <= 500 and read_size - end <= 500:
            return [(0, read_size)]
    mranges.sort(key=lambda m: (m[0], -m[1]))          # CmpMappingRangeBySoff, :110-116: start ascending, end descending
    nr = len(mranges)
    i = 0
    left = mranges[0][0]
    while i < nr:
        j = i + 1
        while j < nr and mranges[j][1] <= mranges[i][1]:          # :138
            j += 1
        if j == nr:
            right = mranges[i][1]
            if float(right - left) >= min_size * 0.95:             # :142
                eranges.append((left, right))
            break
        if mranges[i][1] - mranges[j][0] < 1000:                   # :145
            right = min(mranges[i][1], mranges[j][0])
            if float(right - left) >= min_size * 0.95:             # :148
                eranges.append((left, right))
            left = max(mranges[i][1], mranges[j][0])
        i = j
    return eranges


def segments(cov, eranges, min_cov, min_size):
    """cov: mat_cnt + ins_cnt per position (ints) -> list of (beg, end), consensus_worker's loop"""
    out = []
    for L, R in eranges:                  # :219-222
        beg = L
        while beg < R:
            while beg < R and cov[beg] < min_cov:                  # :225
                beg += 1
            end = beg + 1
            while end < R and cov[end] >= min_cov:                 # :227
                end += 1
            if float(end - beg) >= 0.95 * min_size:                # :228
                out.append((beg, end))
            beg = end
    return out


def windows(ident, cov, beg, end):
    """meap_consensus_one_segment on positions [beg, end) -> (number of anchors, list of (sb, se, cov) that go to meap_cns_one_indel)"""
    out = []
    n = end - beg
    anchors = 0
    i = 0
    while i < n and not (ident[beg + i] & FMAT):                   # :91
        i += 1
    while i < n:                                                   # :92
        anchors += 1
        j = i + 1
        while j < n and not (ident[beg + j] & FMAT):               # :96
            j += 1
        need = False
        for k in range(i, j):                                      # :99-100
            if (ident[beg + k] & UNDS) or (ident[beg + k] & FDEL):
                need = True
                break
        if need:
            out.append((i + beg, j + beg, cov[beg + i]))           # :103
        i = j
    return anchors, out


def plan(templates, tech, min_cov, min_size):
    """templates: list of (table [TABLE_DTYPE-like with mat_cnt / ins_cnt], ident uint8, mranges) -> the dict mecat_amd.hip returns:
    segments, seg_begin, windows, eranges [k, 2], erange_begin"""
    assert min_size >= 2 and min_cov >= 1
    segs, wins, ers, seg_begin, er_begin = [], [], [], [0], [0]
    for t, (table, ident, mranges) in enumerate(templates):
        cov = (np.asarray(table["mat_cnt"]).astype(np.int64) + np.asarray(table["ins_cnt"]).astype(np.int64)).tolist()
        idl = np.asarray(ident).tolist()
        er = effective_ranges(mranges, len(cov), tech, min_size)
        ers += er
        er_begin.append(len(ers))
        for beg, end in segments(cov, er, min_cov, min_size):
            anchors, w = windows(idl, cov, beg, end)
            segs.append((t, beg, end, anchors, len(wins), len(wins) + len(w)))
            wins += [(sb, se, c, len(segs) - 1) for sb, se, c in w]
        seg_begin.append(len(segs))
    return dict(segments=np.array(segs, dtype=SEGMENT_DTYPE) if segs else np.zeros(0, SEGMENT_DTYPE), seg_begin=np.array(seg_begin, np.int64),
                windows=np.array(wins, dtype=WINDOW_DTYPE) if wins else np.zeros(0, WINDOW_DTYPE),
                eranges=np.array(ers, np.int32).reshape(-1, 2), erange_begin=np.array(er_begin, np.int64))


def same_plan(a, b):
    """None, or a short description of the first difference between two plan dicts"""
    for k in ("erange_begin", "eranges", "seg_begin", "segments", "windows"):
        x, y = a[k], b[k]
        if x.shape != y.shape:
            return "%s: shapes %s / %s" % (k, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            bad = np.nonzero(x != y)[0][:5] if x.dtype.names else np.argwhere(x != y)[:5].tolist()
            return "%s differs at %s: %s / %s" % (k, bad, x[bad[0]] if x.dtype.names else "", y[bad[0]] if x.dtype.names else "")
    return None
