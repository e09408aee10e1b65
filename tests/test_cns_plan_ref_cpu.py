"""tests/cns_plan_ref.py — the restatement of get_effective_ranges, consensus_worker's coverage runs and meap_consensus_one_segment's
anchor walk (mecat2cns/mecat_correction.cpp:118-153, :203-239, :81-108) — on plans computed by hand and written out here.  The
restatement is the checker of the device plan (test_gpu_cns_plan.py); this file is what holds the restatement itself."""
import os

import numpy as np

import cns_plan_ref as P
import cns_table_ref as R
import helpers as H

F, D, I, U = P.FMAT, P.FDEL, P.FINS, P.UNDS


def test_whole_read_shortcut():
    # one alignment within 500 bases of both ends: (0, L), whatever the others are and whatever min_size is   (:124-129)
    assert P.effective_ranges([(3000, 4000), (500, 9500)], 10000, 0, 5000) == [(0, 10000)]
    assert P.effective_ranges([(3000, 4000), (500, 9500)], 10000, 0, 10 ** 6) == [(0, 10000)]
    # 501 at the start, or 501 left at the end: no shortcut; the sweep gives the alignment's own range
    assert P.effective_ranges([(501, 9500)], 10000, 0, 5000) == [(501, 9500)]
    assert P.effective_ranges([(500, 9499)], 10000, 0, 5000) == [(500, 9499)]
    assert P.effective_ranges([(501, 9500)], 10000, 0, 10 ** 6) == []


def test_nothing_accepted_and_nanopore():
    assert P.effective_ranges([], 10000, 0, 5000) == []                    # :122
    assert P.effective_ranges([], 10000, 1, 2000) == [(0, 10000)]           # :509: always the whole read
    assert P.effective_ranges([(3000, 4000)], 10000, 1, 2000) == [(0, 10000)]
    assert P.effective_ranges([], 0, 1, 2000) == [] and P.effective_ranges([], 0, 0, 5000) == []      # no candidates: no table, no range


def test_contained_range_and_equal_starts():
    # sorted: (1000, 9000), (2000, 5000), (8500, 15000).  (2000, 5000) ends inside the first and is stepped over (:138); the first and the
    # third overlap by 500 < 1000: cut at min(9000, 8500) = 8500, go on from max = 9000 (:145-150); the last one closes (:139-143)
    assert P.effective_ranges([(8500, 15000), (2000, 5000), (1000, 9000)], 20000, 0, 2000) == [(1000, 8500), (9000, 15000)]
    # equal starts: the longer one first, the shorter one is contained; equal pairs likewise
    assert P.effective_ranges([(1000, 5000), (1000, 8000)], 20000, 0, 2000) == [(1000, 8000)]
    assert P.effective_ranges([(1000, 8000), (1000, 8000)], 20000, 0, 2000) == [(1000, 8000)]


def test_overlap_999_against_1000():
    # 10000 - 9001 = 999 < 1000: two ranges, (1000, 9001) and (10000, 20000)
    assert P.effective_ranges([(1000, 10000), (9001, 20000)], 30000, 0, 2000) == [(1000, 9001), (10000, 20000)]
    # 10000 - 9000 = 1000: no cut, `left` stays 1000 and the last alignment closes (1000, 20000)
    assert P.effective_ranges([(1000, 10000), (9000, 20000)], 30000, 0, 2000) == [(1000, 20000)]
    # no overlap at all (a gap): negative difference < 1000, right = min = 10000, left = max = 12000
    assert P.effective_ranges([(1000, 10000), (12000, 20000)], 30000, 0, 2000) == [(1000, 10000), (12000, 20000)]


def test_kept_and_dropped_remainder():
    # min_size 2000: right - left >= 1900.0
    assert P.effective_ranges([(1000, 2900)], 30000, 0, 2000) == [(1000, 2900)]
    assert P.effective_ranges([(1000, 2899)], 30000, 0, 2000) == []
    # the piece in front of a cut is dropped (right = min(2899, 2000) = 2000: 1000 positions), the one behind it kept:
    # left = max(2899, 2000) = 2899, 4799 - 2899 = 1900
    assert P.effective_ranges([(1000, 2899), (2000, 4799)], 30000, 0, 2000) == [(2899, 4799)]
    # ... and the other way round: (1000, 2950) kept (1950), then left = 3000 and 4899 - 3000 = 1899 is one short
    assert P.effective_ranges([(1000, 3000), (2950, 4899)], 30000, 0, 2000) == [(1000, 2950)]
    # both short: 2000 - 1000 = 1000, then 4799 - 2900 = 1899
    assert P.effective_ranges([(1000, 2900), (2000, 4799)], 30000, 0, 2000) == []
    # min_size 3: 2.85 — three positions are enough, two are not (a threshold that is no integer)
    assert P.effective_ranges([(1000, 1003)], 30000, 0, 3) == [(1000, 1003)]
    assert P.effective_ranges([(1000, 1002)], 30000, 0, 3) == []


def test_runs_at_the_threshold():
    # min_size 20: end - beg >= 19.0.  Runs of 19 (kept), 18 (dropped), 20 (kept); coverage min_cov - 1 breaks a run
    cov = [0] * 5 + [4] * 19 + [3] * 3 + [4] * 18 + [0] + [9] * 20 + [3]
    assert len(cov) == 67
    assert P.segments(cov, [(0, 67)], 4, 20) == [(5, 24), (46, 66)]
    assert P.segments(cov, [(0, 67)], 5, 20) == [(46, 66)]
    # min_size 21: 19.95 — 20 positions kept, 19 dropped
    assert P.segments(cov, [(0, 67)], 4, 21) == [(46, 66)]
    # a run that reaches the end of the range
    assert P.segments([4] * 30, [(0, 30)], 4, 20) == [(0, 30)]
    # nothing covered: beg reaches R, end = R + 1, 1 < 1.9
    assert P.segments([0] * 30, [(0, 30)], 4, 2) == []
    # min_size 2: 1.9 — single covered positions are no segments, pairs are
    assert P.segments([4, 0, 4, 4, 0, 4, 4, 4], [(0, 8)], 4, 2) == [(2, 4), (5, 8)]


def test_ranges_cut_runs():
    cov = [5] * 60
    # two ranges that touch inside one covered run: the reference restarts at the second range's start (:221-223)
    assert P.segments(cov, [(0, 30), (30, 60)], 4, 20) == [(0, 30), (30, 60)]
    assert P.segments(cov, [(0, 30), (30, 60)], 4, 40) == []
    assert P.segments(cov, [(0, 60)], 4, 40) == [(0, 60)]
    # a range that ends in the middle of a run: the run ends with it
    assert P.segments(cov, [(10, 29)], 4, 20) == [(10, 29)]
    assert P.segments(cov, [(10, 28)], 4, 20) == []


def test_counts_are_unsigned_bytes_summed_as_int():
    table = np.zeros(4, R.TABLE_DTYPE)
    table["mat_cnt"] = 100
    table["ins_cnt"] = 100
    p = P.plan([(table, np.full(4, F, np.uint8), [])], 1, 200, 4)
    assert p["segments"].tolist() == [(0, 0, 4, 4, 0, 0)]
    assert len(P.plan([(table, np.full(4, F, np.uint8), [])], 1, 201, 4)["segments"]) == 0


def test_anchor_walk_by_hand():
    #        0  1  2  3  4  5  6  7  8      9  10 11 12 13 14 15
    ident = [U, F, U, I, F, F, U, I, F | D, F, F, I, F, D, F, U]
    cov = list(range(10, 26))
    # segment [2, 14): anchors 4, 5, 8, 9, 10, 12.  Position 2 (UNDS) lies in front of the first anchor: nothing.
    # (4, 5) clean; (5, 8) holds UNDS at 6; (8, 9) is dirty at its own anchor (FMAT | FDEL); (9, 10) clean; (10, 12) holds FINS only: clean;
    # (12, 14): no anchor behind 12, so it ends with the segment, and 13 has FDEL
    assert P.windows(ident, cov, 2, 14) == (6, [(5, 8, 15), (8, 9, 18), (12, 14, 22)])
    # the same table, the segment one longer: 14 is an anchor, the last window (14, 15) is clean, (12, 14) stays
    assert P.windows(ident, cov, 2, 15) == (7, [(5, 8, 15), (8, 9, 18), (12, 14, 22)])
    # a segment without anchors; dirty positions in front of the only anchor; an anchor at the very end
    assert P.windows([U, U, I, D], [5] * 4, 0, 4) == (0, [])
    assert P.windows([U, D, U, F], [5] * 4, 0, 4) == (1, [])
    assert P.windows([F, U, U, U], [7, 5, 5, 5], 0, 4) == (1, [(0, 4, 7)])


def test_plan_numbers_segments_and_windows_across_templates():
    def tmpl(cov, ident):
        t = np.zeros(len(cov), R.TABLE_DTYPE)
        t["mat_cnt"] = cov
        return t, np.array(ident, np.uint8)
    a = tmpl([4, 4, 4, 0, 4, 4, 4, 4], [F, U, F, F, F, D, F, U])          # segments (0, 3) and (4, 8)
    b = tmpl([0, 0, 0], [F, F, F])                                          # nothing covered
    c = tmpl([9, 9, 9, 9], [U, F | D, U, U])                                # one segment, one window (1, 4)
    p = P.plan([a + ([],), b + ([],), (np.zeros(0, R.TABLE_DTYPE), np.zeros(0, np.uint8), []), c + ([],)], 1, 4, 3)
    assert p["erange_begin"].tolist() == [0, 1, 2, 2, 3] and p["eranges"].tolist() == [[0, 8], [0, 3], [0, 4]]
    assert p["seg_begin"].tolist() == [0, 2, 2, 2, 3]
    assert p["segments"].tolist() == [(0, 0, 3, 2, 0, 1), (0, 4, 8, 2, 1, 3), (3, 0, 4, 1, 3, 4)]
    assert p["windows"].tolist() == [(0, 2, 4, 0), (4, 6, 4, 1), (6, 8, 4, 1), (1, 4, 9, 2)]
    assert P.same_plan(p, p) is None
    q = {k: v.copy() for k, v in p.items()}
    q["windows"]["cov"][2] = 5
    assert "windows" in P.same_plan(p, q)


def test_the_recorded_tables_give_the_pipeline_test_something_to_test():
    """the sixteen templates whose reference tables tests/golden/cns_table.npz holds in full, at the mecat2cns defaults: at least half of
    them yield a segment, and together they yield at least 1 000 windows (the conditions test_gpu_cns_plan.py asserts on the device)"""
    import cns_table_golden as TG
    T = TG.golden()
    G = np.load(os.path.join(H.GOLDEN, "cns_accept.npz"))
    with_seg = nwin = 0
    for name, tech in (("pacbio", 0), ("nanopore", 1)):
        assert int(G[name + "_par"][5]) == tech
        table, ident, b8 = TG.planes_to_table(T[name + "_table8"]), T[name + "_ident8"], T[name + "_begin8"]
        first = np.concatenate([[0], np.cumsum(G[name + "_nacc"])])
        tm = [(table[b8[t]: b8[t + 1]], ident[b8[t]: b8[t + 1]], G[name + "_meta"][first[t]: first[t + 1], :2]) for t in range(8)]
        p = P.plan(tm, tech, *P.DEFAULTS[tech])
        with_seg += int((np.diff(p["seg_begin"]) > 0).sum())
        nwin += len(p["windows"])
    assert with_seg >= 8 and nwin >= 1000, (with_seg, nwin)
