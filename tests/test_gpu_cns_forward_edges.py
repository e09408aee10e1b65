"""The mecat2cns re-aligner's forward pass (cns_forward = dw_extend2<true>) and cns_trace against the oracle restatement (orc_cns_dw,
orc_cns_get_alignment: dw-level coordinates, column and indel counts, `ok`, the GetAlignment coordinates and both aligned strings rebuilt
from the 2-bit columns), with a block size, a band width, a record group or a hand-over reason placed at its edge on purpose.  Every job
list also runs with MECAT_CNS_KERNEL=1 (every unit through cns_extend): results and every column word byte-equal to the default path's.

1. Block rule edges (dw.cpp:319-332): last blocks of ext = 1..64, 496, 499, 500, 501, 511, 512, 513, 527, 528, 529, 599, 600 bases and
   601 (a full block plus a rest) on the shorter side of both directions of a job, the other sequence 1.0 x and 1.3 x as long, both
   strands, reads at error 0, 0.05 and 0.15, run under error_rate 0.15 and 0.20 and min_align_size 1 and 500; start points 0 and
   size - 1.  Behind one full block (whose advance is computed with the oracle's block routine, 496 for identical sequences) a rest is
   always more than 100 bases (a full block is only taken while more than 600 are left and advances by at most 500): the sizes 496 ..
   601 stand behind a full block, and so do the smallest rests there are (601 .. 604 bases in all); 1 .. 64 cannot.
2. Wide rows: one insertion of 40, 70 or 90 bases in the query or the target, 60 - 400 bases behind the seed point on either side,
   reads at error 0, 0.05 and 0.15, both strands (rows of two and three passes: `hi` and `top` of a row record); insertions of
   29 .. 35 and 61 .. 67 bases right behind the seed point of clean reads, followed by 0, 1 or 2 substitutions: the block's end row and
   the widest rows lie at rows 29 .. 39 and 61 .. 71, around the 32-row words of cns_trace's path array.
3. Record groups and staging history: ~3 000 jobs on ~1 000 pairs of 1 - 3 kb with seed points at piece boundaries, mixed with the
   lists of 1 and 2; in the given order, in a permuted order and behind one extra leading job (three of them, whose shares shift every
   later unit's first row record by 1, 2 and 3 modulo cns_trace's aligned groups of four), each at the default wave count and with
   MECAT_CNS_WAVES=4.  The given order at the default wave count is checked against the oracle job by job; every other run must
   reproduce it byte for byte, results and column words.
4. Every hand-over reason, each group in a call of its own, with the number of units the forward pass handed over read from debug
   counter 8 (dw_extend2 adds `nhand` there: one per unit it puts on the hand-over list, for whatever reason, over all slices of the
   call; nothing else in a re-aligner call touches the slot, and with MECAT_CNS_KERNEL=1 it stays 0).  Observed on an MI355X, units
   handed over of the units of the group (two per job):
     row log share   12 pairs with 6 - 10 kb arms, run at error_rate 0.15.  The reads carry 0.30 - 0.32 error of this file's
                     mix, which the aligner crosses in 0.45 - 0.49 rows per base: more than the share's 2.7 e = 0.405, less
                     than a block's max_d of 4 e = 0.6 (at 0.22 - 0.28 it is 0.37 - 0.45 rows and few units outgrow the share;
                     the oracle's block routine predicts 20 of the 24 on the CPU)                                         24 of 24
     wide row        24 pairs with an insertion of 110 or 140 bases in one direction: rows of more than 96 diagonals.  The
                     pass count of a row is the wave's, so the unit in the other half of the wave is handed over with it   32 of 48
     ring            24 pairs, one direction with a substitution at every third base over the 120 - 141 bases in front of
                     the first full block's end (and the 8 behind it), clean around them: ~47 substitutions are at most 95
                     rows, of at most 96 diagonals; the path leaves the main diagonal there, and where its last dozen rows —
                     what the ring holds of rows 70 - 90 diagonals wide — have no run of four matches the tail walk is lost   11 of 48
     block records   24 pairs of 2.4 - 3 kb, reads at error 0 and 0.05, under MECAT_CNS_BLOCK_SHARE=12,2: two records a
                     unit, three blocks a direction                                                                      48 of 48
     control         16 identical pairs of 1.5 kb                                                                          0 of 32
     96 diagonals    16 clean pairs with an insertion of 95 bases right behind the seed point: row d of a block has at
                     most d + 1 diagonals and an end is reached in row 95 at the latest, so no row passes 96               0 of 32
   (Groups 1 - 3 for comparison: 0 of 2 544 units of the block edges, 128 of 744 of the wide rows — insertions of 90 bases in reads
   with errors of their own, and their neighbours in the wave.)
5. The column cap: identical reads with exactly 512 / 513 columns in the right (left) direction under dir_cols_cap = 512.
"""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

CAP = 8192                      # columns per direction: the reads of groups 1 - 3 stay under 4.3 kb
EDGES = tuple(range(1, 65)) + (496, 499, 500, 501, 511, 512, 513, 527, 528, 529, 599, 600, 601)
READ_ERRORS = (0.0, 0.05, 0.15)
SEG = 500                       # mecat2cns' full block


@pytest.fixture(scope="module")
def hip():
    import mecat_amd.hip as M
    return M


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------- sequences
def _mutate(rng, s, e):
    """substitutions, deletions and insertions at a total rate of about e (the mix of test_gpu_dw_doubled._mutate), vectorised"""
    if e == 0.0:
        return s.astype(np.int8)
    u = rng.random(len(s))
    keep = u >= 0.25 * e
    b = np.where(u < 0.4 * e, rng.integers(0, 4, size=len(s)), s)[keep]
    reps = 1 + (rng.random(len(b)) < 0.6 * e)
    out = np.repeat(b, reps)
    ins = np.cumsum(reps) - 1                      # the second copy of a doubled base becomes a random base
    ins = ins[reps == 2]
    out[ins] = rng.integers(0, 4, size=len(ins))
    return out.astype(np.int8)


def _arm(rng, nq, nt, e):
    """the two sequences of one direction, read away from the seed point: nq and nt bases of two copies of one stretch"""
    n = max(nq, nt)
    g = rng.integers(0, 4, size=2 * n + 64).astype(np.int8)
    q, t = _mutate(rng, g, e), _mutate(rng, g, e)
    assert len(q) >= nq and len(t) >= nt
    return q[:nq], t[:nt]


def _join(left, right):
    """(q, t, qstart, tstart) from the two arms (query bases, target bases) on either side of the seed point"""
    (ql, tl), (qr, tr) = left, right
    return np.concatenate([ql[::-1], qr]).astype(np.int8), np.concatenate([tl[::-1], tr]).astype(np.int8), len(ql), len(tl)


def _arm_with_insertion(rng, n, e, at, ins, in_query, subs=0):
    """an arm of about n bases with `ins` extra bases in one sequence `at` bases behind the seed point, and `subs` single substitutions
    10 and 20 bases behind the insertion"""
    g = rng.integers(0, 4, size=n).astype(np.int8)
    q = [_mutate(rng, g[:at], e), _mutate(rng, g[at:], e)]
    t = [_mutate(rng, g[:at], e), _mutate(rng, g[at:], e)]
    for i in range(subs):
        q[1][10 * (i + 1)] = (q[1][10 * (i + 1)] + 1) & 3
    extra = rng.integers(0, 4, size=ins).astype(np.int8)
    side = q if in_query else t
    side[1] = np.concatenate([extra, side[1]])
    return np.concatenate(q), np.concatenate(t)


def _arm_with_dirty_block_end(rng, n, width):
    """a clean arm of n bases whose last `width` bases in front of the first full block's end (and the eight behind it) carry a
    substitution at every third base: no run of four matches there"""
    q = rng.integers(0, 4, size=n).astype(np.int8)
    t = q.copy()
    at = np.arange(SEG - width, SEG + 8, 3)
    t[at] = (t[at] + 1 + rng.integers(0, 3, size=len(at))) & 3
    return q, t


# ----------------------------------------------------------------------------- the oracle
class _Orc:
    def __init__(self):
        self.O = H.orc()
        self.a = self.O.orc_cns_new()
        self.s1, self.s2 = np.zeros(100001, np.int8), np.zeros(100001, np.int8)
        self.bops = np.zeros(8192, np.uint8)

    def job(self, q, qs, t, ts, er, mn):
        """what _check wants of one job: (ok, res[9], ok2, res2[5], qaln, saln)"""
        O, a, s1, s2 = self.O, self.a, self.s1, self.s2
        res, res2 = np.zeros(9, np.int32), np.zeros(5, np.int32)
        ok = O.orc_cns_dw(a, q.ctypes.data, qs, len(q), t.ctypes.data, ts, len(t), er, mn, res.ctypes.data, s1.ctypes.data, s2.ctypes.data)
        ok2 = O.orc_cns_get_alignment(a, q.ctypes.data, qs, len(q), t.ctypes.data, ts, len(t), er, mn, res2.ctypes.data, s1.ctypes.data, s2.ctypes.data)
        return ok, res, ok2, res2, s1[: res2[4]].tobytes(), s2[: res2[4]].tobytes()

    def full_block_advance(self, q, t, er=0.20):
        """what a first full block of the arms q, t (read away from the seed point) advances by in either sequence: the block's columns
        in front of its last run of four matches (dw.cpp:333-373); None when the block ends the direction"""
        import ctypes as C
        O = self.O
        O.orc_cns_align_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 5
        q, t = np.ascontiguousarray(q[:SEG], dtype=np.int8), np.ascontiguousarray(t[:SEG], dtype=np.int8)
        out = np.zeros(4, np.int32)
        p = out.ctypes.data
        if not O.orc_cns_align_block(self.a, q.ctypes.data, t.ctypes.data, SEG, 1, er, p, p + 4, p + 8, self.bops.ctypes.data, p + 12):
            return None
        qe, te, _, n = (int(x) for x in out)
        i = j = nm = 0
        for k in range(n - 1, -1, -1):
            if nm == 4:
                break
            op = int(self.bops[k])
            i += op != 1
            j += op != 2
            nm = nm + 1 if op == 0 else 0
        i, j = SEG - qe + i, SEG - te + j
        return None if i == SEG else (SEG - i, SEG - j)

    def close(self):
        self.O.orc_cns_free(self.a)


class _Jobs:
    """a job list over a volume of its own; the oracle's answers per (error_rate, min_align_size), computed once and kept"""

    def __init__(self):
        self.seqs, self.jobs, self.metas, self._want = [], [], [], {}

    def add_pair(self, q, t):
        """-> the pair's number; its query is stored once per strand it is used on"""
        self.seqs.append([np.ascontiguousarray(q, dtype=np.int8), np.ascontiguousarray(t, dtype=np.int8), None, None, None])
        return len(self.seqs) - 1

    def add(self, pair, qs, ts, chain):
        self.jobs.append((pair, qs, ts, chain))

    def add_new(self, q, t, qs, ts, chain):
        self.add(self.add_pair(q, t), qs, ts, chain)

    def extend(self, other):
        base = len(self.seqs)
        self.seqs += [list(s) for s in other.seqs]
        self.jobs += [(p + base, qs, ts, chain) for p, qs, ts, chain in other.jobs]

    def __len__(self):
        return len(self.jobs)

    def volume(self, hip, ctx):
        """-> (volume, job array): the volume holds a read as sequenced, so a job on strand 1 names the reverse complement of its query"""
        reads = []
        for s in self.seqs:
            s[2] = s[3] = s[4] = None
        for pair, _, _, chain in self.jobs:
            s = self.seqs[pair]
            if s[2 + chain] is None:
                s[2 + chain] = len(reads)
                reads.append((3 - s[0][::-1]).astype(np.int8) if chain else s[0])
            if s[4] is None:
                s[4] = len(reads)
                reads.append(s[1])
        reads.append(np.zeros(64, np.int8))                          # (no job's read is the last of the volume)
        lens = np.array([len(r) for r in reads], dtype=np.int32)
        ov = H.orc_pack(np.concatenate(reads).astype(np.uint8), lens)
        offs, pac = H.vol_arrays(ov)
        num_bases = ov.contents.num_bases
        H.orc().orc_volume_free(ov)
        ja = np.zeros(len(self.jobs), dtype=hip.JOB_DTYPE)
        for i, (pair, qs, ts, chain) in enumerate(self.jobs):
            s = self.seqs[pair]
            ja[i] = (s[2 + chain], s[4], chain, qs, ts)
        return hip.Volume(ctx, pac, offs, num_bases, 0), ja

    def want(self, orc, er, mn):
        if (er, mn) not in self._want:
            self._want[(er, mn)] = [orc.job(self.seqs[p][0], qs, self.seqs[p][1], ts, er, mn) for p, qs, ts, _ in self.jobs]
        return self._want[(er, mn)]

    def longest(self):
        return max(max(len(s[0]), len(s[1])) for s in self.seqs)


def _check(hip, r, ops_row, q, t, want):
    """test_gpu_cns._check"""
    ok, res, ok2, res2, qaln, saln = want
    # dw level: coordinates, column count, indel counts of the untrimmed string (the reference only fills the counts on success)
    assert (int(r["query_start"]), int(r["query_end"]), int(r["target_start"]), int(r["target_end"])) == tuple(int(x) for x in res[:4])
    assert int(r["left_cols"]) + int(r["right_cols"]) == int(res[4])
    if ok:
        assert (int(r["mat"]), int(r["ins"]), int(r["dele"])) == (int(res[5]), int(res[7]), int(res[8]))
    # GetAlignment level
    assert int(r["ok"]) == int(ok2)
    if ok2:
        assert (int(r["qoff"]), int(r["qend"]), int(r["soff"]), int(r["send"])) == tuple(int(x) for x in res2[:4])
        assert int(r["last_col"]) - int(r["first_col"]) == int(res2[4])
        gq, gs = hip.cns_expand(r, ops_row, q, t)
        assert gq == qaln and gs == saln


def _check_all(hip, J, res, ops, want, what):
    assert len(res) == len(J.jobs) == len(want)
    for i, (pair, qs, ts, chain) in enumerate(J.jobs):
        q, t = J.seqs[pair][0], J.seqs[pair][1]
        try:
            _check(hip, res[i], ops[i], q, t, want[i])
        except AssertionError:
            print(what, "job", i, "n", len(q), len(t), "qs", qs, "ts", ts, "chain", chain, "gpu", res[i], "orc", want[i][:4])
            raise


def _share_ok2(want):
    return sum(int(w[2]) for w in want) / max(len(want), 1)


ENV = ("MECAT_CNS_KERNEL", "MECAT_CNS_WAVES", "MECAT_CNS_BLOCK_SHARE", "MECAT_CNS_LOG_GB", "MECAT_TRACE")


def _run(hip, ctx, monkeypatch, vol, ja, er, mn, cap=CAP, **env):
    """one call with exactly the given knobs set -> (results, column words, units the forward pass handed over)"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx.reset_stats()
    try:
        res, ops = hip.cns_align_candidates(ctx, vol, vol, ja, er, mn, cap)
        handed = ctx.debug_counter(8)
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
    return res, ops, handed


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ----------------------------------------------------------------------------- the job lists
def _block_edge_jobs(orc):
    rng = np.random.default_rng(31907)
    J = _Jobs()

    def behind_full_block(e, rest, ratio):
        """an arm whose first block is a full one and leaves `rest` bases of the shorter sequence, rest * ratio of the other"""
        q, t = _arm(rng, 1400, 1400, e)
        adv = orc.full_block_advance(q, t) or (SEG - 4, SEG - 4)
        return q[: adv[0] + rest], t[: adv[1] + int(round(rest * ratio))]

    def both_ways(left, right, chain):
        # the query is the shorter side on the left of the seed point, the target on the right; then the two swapped, on the other strand
        q, t, qs, ts = _join(left, (right[1], right[0]))
        J.add_new(q, t, qs, ts, chain)
        J.add_new(t, q, ts, qs, 1 - chain)

    for e in READ_ERRORS:
        for n in EDGES:
            for ratio in (1.0, 1.3):
                chain = (n + int(ratio > 1)) & 1
                long_ = int(round(n * ratio))
                both_ways(_arm(rng, n, long_, e), _arm(rng, n, long_, e), chain)
                if n >= 496:
                    both_ways(behind_full_block(e, n, ratio), behind_full_block(e, n, ratio), 1 - chain)
        # the smallest rests behind a full block: 601 .. 604 bases in all
        for total in (601, 602, 603, 604):
            both_ways(_arm(rng, total, total, e), _arm(rng, total, int(total * 1.3), e), total & 1)
    # empty and one-base directions: start points 0 and size - 1, on pairs whose other direction aligns
    for e in READ_ERRORS:
        for n in (3, 40, 700, 1300):
            q, t = _arm(rng, n, n + 100, e)
            for chain in (0, 1):
                p = J.add_pair(q, t)
                J.add(p, 0, 0, chain)
                J.add(p, len(q) - 1, len(q) - 1, chain)
                J.add(p, 0, min(7, len(t) - 1), chain)
                J.add(p, min(7, len(q) - 1), 0, chain)
                p = J.add_pair(q[::-1].copy(), t[::-1].copy())           # (the common stretch at the reads' ends)
                J.add(p, len(q) - 1, len(t) - 1, chain)
                J.add(p, len(q) - 2 if n > 3 else 0, len(t) - 1, chain)
                J.add(p, len(q) - 1, len(t) - 2, chain)
    return J


def _wide_row_jobs():
    rng = np.random.default_rng(271828)
    J = _Jobs()
    # one insertion of 40 / 70 / 90 bases, 60 - 400 bases behind the seed point on either side
    for it in range(144):
        e = READ_ERRORS[it % 3]
        ins = (40, 70, 90)[(it // 3) % 3]
        at = int(rng.integers(60, 400))
        n = int(rng.integers(700, 1400))
        wide = _arm_with_insertion(rng, n, e, at, ins, bool(it & 16))
        plain = _arm(rng, int(rng.integers(500, 1400)), int(rng.integers(500, 1400)), e)
        q, t, qs, ts = _join(wide, plain) if it & 8 else _join(plain, wide)
        p = J.add_pair(q, t)
        for chain in (0, 1):
            J.add(p, qs, ts, chain)
    # clean reads, the insertion right behind the seed point and 0 - 2 substitutions behind it: end rows 29 .. 39 and 61 .. 71
    it = 0
    for ins in tuple(range(29, 36)) + tuple(range(61, 68)):
        for subs in (0, 1, 2):
            for in_query in (False, True):
                wide = _arm_with_insertion(rng, 900, 0.0, 12, ins, in_query, subs)
                plain = _arm(rng, 300, 300, 0.0)
                q, t, qs, ts = _join(wide, plain) if it & 1 else _join(plain, wide)
                J.add_new(q, t, qs, ts, (it >> 1) & 1)
                it += 1
    return J


def _history_jobs():
    """test_gpu_dw_block_setup.test_results_do_not_depend_on_staging_history's pairs"""
    rng = np.random.default_rng(4711)
    J = _Jobs()
    for it in range(1000):
        e = (0.15, 0.15, 0.05, 0.0)[it % 4]
        cuts = np.sort(rng.integers(0, int(rng.integers(1000, 2400)), size=3))
        L = int(rng.integers(int(cuts[2]) + 1, int(cuts[2]) + 700))
        g = rng.integers(0, 4, size=L).astype(np.int8)
        qp = [_mutate(rng, p, e) for p in np.split(g, cuts)]
        tp = [_mutate(rng, p, e) for p in np.split(g, cuts)]
        if it % 10 == 0:
            tp[3] = tp[3][: len(tp[3]) // 2]             # unequal rests
        if it % 10 == 5:
            qp[0] = qp[0][len(qp[0]) // 3:]
        q, t = np.concatenate(qp), np.concatenate(tp)
        if len(q) < 20 or len(t) < 20:
            continue
        p = J.add_pair(q, t)
        for k in (1, 2, 3):                                  # seed points at the piece boundaries: they correspond exactly
            qs, ts = sum(len(x) for x in qp[:k]), sum(len(x) for x in tp[:k])
            J.add(p, min(qs, len(q) - 1), min(ts, len(t) - 1), (it + k) & 1)
    return J


def _rowlog_jobs():
    rng = np.random.default_rng(1618)
    J = _Jobs()
    for it in range(12):
        e = (0.30, 0.32)[it & 1]
        left = _arm(rng, int(rng.integers(6000, 10000)), int(rng.integers(6000, 10000)), e)
        right = _arm(rng, int(rng.integers(6000, 10000)), int(rng.integers(6000, 10000)), e)
        q, t, qs, ts = _join(left, right)
        J.add_new(q, t, qs, ts, (it >> 1) & 1)
    return J


def _too_wide_jobs():
    rng = np.random.default_rng(1414)
    J = _Jobs()
    for it in range(24):
        e = READ_ERRORS[it % 3]
        wide = _arm_with_insertion(rng, int(rng.integers(900, 1400)), e, int(rng.integers(60, 300)), (110, 140)[(it // 3) & 1], bool(it & 8))
        plain = _arm(rng, 800, 800, e)
        q, t, qs, ts = _join(wide, plain) if it & 4 else _join(plain, wide)
        J.add_new(q, t, qs, ts, it & 1)
    return J


def _ring_jobs():
    rng = np.random.default_rng(2236)
    J = _Jobs()
    for it in range(24):
        dirty = _arm_with_dirty_block_end(rng, int(rng.integers(1100, 1600)), int(rng.integers(120, 142)))
        plain = _arm(rng, 700, 700, 0.0)
        if it & 2:
            dirty = (dirty[1], dirty[0])
        q, t, qs, ts = _join(dirty, plain) if it & 4 else _join(plain, dirty)
        J.add_new(q, t, qs, ts, it & 1)
    return J


def _block_record_jobs():
    rng = np.random.default_rng(1732)
    J = _Jobs()
    for it in range(24):
        e = (0.0, 0.05)[it & 1]
        left = _arm(rng, int(rng.integers(1200, 1500)), int(rng.integers(1200, 1500)), e)
        right = _arm(rng, int(rng.integers(1200, 1500)), int(rng.integers(1200, 1500)), e)
        q, t, qs, ts = _join(left, right)
        J.add_new(q, t, qs, ts, (it >> 1) & 1)
    return J


def _control_jobs():
    rng = np.random.default_rng(3)
    J = _Jobs()
    for it in range(16):
        g = rng.integers(0, 4, size=1500).astype(np.int8)
        J.add_new(g, g.copy(), 750 - 40 * it, 750 - 40 * it, it & 1)
    return J


def _row_of_96_jobs():
    rng = np.random.default_rng(96)
    J = _Jobs()
    for it in range(16):
        wide = _arm_with_insertion(rng, 1000, 0.0, 12, 95, bool(it & 2))
        plain = _arm(rng, 400, 400, 0.0)
        q, t, qs, ts = _join(wide, plain) if it & 4 else _join(plain, wide)
        J.add_new(q, t, qs, ts, it & 1)
    return J


@pytest.fixture(scope="module")
def orc():
    o = _Orc()
    yield o
    o.close()


@pytest.fixture(scope="module")
def lists(orc):
    """the lists of groups 1 - 3, built once"""
    edges, wide, hist = _block_edge_jobs(orc), _wide_row_jobs(), _history_jobs()
    mixed = _Jobs()
    for part in (hist, edges, wide):
        mixed.extend(part)
    order = np.random.default_rng(8128).permutation(len(mixed))          # mixed, not one behind the other
    mixed.jobs = [mixed.jobs[i] for i in order]
    return {"edges": edges, "wide": wide, "mixed": mixed}


# ----------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("error_rate,min_align", [(0.15, 1), (0.15, 500), (0.20, 1), (0.20, 500)])
def test_block_rule_edges(hip, ctx, orc, lists, monkeypatch, error_rate, min_align):
    J = lists["edges"]
    assert J.longest() <= 4300
    want = J.want(orc, error_rate, min_align)
    vol, ja = J.volume(hip, ctx)
    got = _run(hip, ctx, monkeypatch, vol, ja, error_rate, min_align)
    one = _run(hip, ctx, monkeypatch, vol, ja, error_rate, min_align, MECAT_CNS_KERNEL="1")
    vol.free()
    _check_all(hip, J, got[0], got[1], want, "block edges")
    assert _same(got, one), "the default path and cns_extend differ"
    # reads shorter than the four-match anchor and blocks with max_d of 0 or 1 are part of the list, and they never align
    tiny = [w for (p, qs, ts, c), w in zip(J.jobs, want) if min(len(J.seqs[p][0]), len(J.seqs[p][1])) <= 3]
    assert len(tiny) >= 12 and not any(w[2] for w in tiny)
    print("block edges: %d jobs, the oracle accepts %.0f %%, %d units handed over" % (len(J), 100 * _share_ok2(want), got[2]))
    if min_align == 1:
        assert _share_ok2(want) >= 1 / 3


@pytest.mark.parametrize("error_rate", [0.15, 0.20])
def test_wide_rows(hip, ctx, orc, lists, monkeypatch, error_rate):
    J = lists["wide"]
    assert J.longest() <= 4300
    want = J.want(orc, error_rate, 500)
    vol, ja = J.volume(hip, ctx)
    got = _run(hip, ctx, monkeypatch, vol, ja, error_rate, 500)
    one = _run(hip, ctx, monkeypatch, vol, ja, error_rate, 500, MECAT_CNS_KERNEL="1")
    vol.free()
    _check_all(hip, J, got[0], got[1], want, "wide rows")
    assert _same(got, one), "the default path and cns_extend differ"
    print("wide rows: %d jobs, the oracle accepts %.0f %%, %d units handed over" % (len(J), 100 * _share_ok2(want), got[2]))
    assert _share_ok2(want) >= 1 / 3


# ----------------------------------------------------------------------------- 3
@pytest.fixture(scope="module")
def history(hip, ctx, orc, lists):
    """the mixed list's volume, its oracle answers and — filled in by the first test that runs — the checked result in the given order"""
    J = lists["mixed"]
    vol, ja = J.volume(hip, ctx)
    state = {"J": J, "vol": vol, "ja": ja, "want": J.want(orc, 0.15, 500), "first": None}
    yield state
    vol.free()


def _first_run(hip, ctx, monkeypatch, S):
    """the given order at the default wave count, checked against the oracle job by job: what every other order and wave count must
    reproduce byte for byte (which makes each of them equal to the oracle job by job as well)"""
    if S["first"] is None:
        got = _run(hip, ctx, monkeypatch, S["vol"], S["ja"], 0.15, 500)
        _check_all(hip, S["J"], got[0], got[1], S["want"], "mixed list")
        S["first"] = got
    return S["first"]


def test_mixed_list_matches_oracle_and_one_unit_kernel(hip, ctx, history, monkeypatch):
    S = history
    assert len(S["J"]) > 4500 and S["J"].longest() <= 4300
    assert _share_ok2(S["want"]) >= 1 / 3
    first = _first_run(hip, ctx, monkeypatch, S)
    one = _run(hip, ctx, monkeypatch, S["vol"], S["ja"], 0.15, 500, MECAT_CNS_KERNEL="1")
    assert _same(first, one), "the default path and cns_extend differ"
    print("mixed list: %d jobs, the oracle accepts %.0f %%, %d units handed over" % (len(S["J"]), 100 * _share_ok2(S["want"]), first[2]))


@pytest.mark.parametrize("waves", [None, "4"])
def test_results_do_not_depend_on_order_or_log_position(hip, ctx, history, monkeypatch, waves):
    S = history
    first = _first_run(hip, ctx, monkeypatch, S)
    env = {"MECAT_CNS_WAVES": waves} if waves else {}
    ja, n = S["ja"], len(S["ja"])
    if waves:
        given = _run(hip, ctx, monkeypatch, S["vol"], ja, 0.15, 500, **env)
        assert _same(given, first), "given order on four waves"
    perm = np.random.default_rng(5040).permutation(n)
    back = np.argsort(perm)
    res, ops, _ = _run(hip, ctx, monkeypatch, S["vol"], ja[perm], 0.15, 500, **env)
    assert _same((res[back], ops[back]), first), "permuted order"
    # one extra job in front: its two units' shares of the row log (cns_caps: 2.7 e of the reach, a block at max_d and 64 rows) move
    # every later unit's first record, by 1, 2 and 3 modulo the groups of four that cns_trace reads
    def shift(job):
        pair, qs, ts, _ = job
        nq, nt = len(S["J"].seqs[pair][0]), len(S["J"].seqs[pair][1])
        return sum(int(2.7 * 0.15 * ext) + int(4.0 * 0.15 * (SEG + 100)) + 64 for ext in (min(qs, ts), min(nq - qs, nt - ts)))
    leads = [next(i for i, job in enumerate(S["J"].jobs) if shift(job) % 4 == r) for r in (1, 2, 3)]
    for lead in leads:
        res, ops, _ = _run(hip, ctx, monkeypatch, S["vol"], np.concatenate([ja[lead: lead + 1], ja]), 0.15, 500, **env)
        assert _same((res[1:], ops[1:]), first), "behind one more job"
        assert res[0] == first[0][lead] and np.array_equal(ops[0], first[1][lead])


# ----------------------------------------------------------------------------- 4
HAND_OVER_GROUPS = {
    # name: (jobs, error_rate, dir_cols_cap, knobs, at least a third accepted)
    "row log share": (_rowlog_jobs, 0.15, 16384, {}, True),
    "wide row": (_too_wide_jobs, 0.15, CAP, {}, False),
    "ring": (_ring_jobs, 0.15, CAP, {}, True),
    "block records": (_block_record_jobs, 0.15, CAP, {"MECAT_CNS_BLOCK_SHARE": "12,2"}, True),
}


@pytest.mark.parametrize("group", list(HAND_OVER_GROUPS))
def test_hand_over_reason_is_taken(hip, ctx, orc, monkeypatch, group):
    build, er, cap, knobs, third = HAND_OVER_GROUPS[group]
    J = build()
    want = J.want(orc, er, 500)
    vol, ja = J.volume(hip, ctx)
    got = _run(hip, ctx, monkeypatch, vol, ja, er, 500, cap, **knobs)
    one = _run(hip, ctx, monkeypatch, vol, ja, er, 500, cap, MECAT_CNS_KERNEL="1")
    vol.free()
    print("%s: %d of %d units handed over, the oracle accepts %.0f %%" % (group, got[2], 2 * len(J), 100 * _share_ok2(want)))
    assert got[2] >= 1, "no unit of the group was handed over: the path was not taken"
    assert one[2] == 0                                   # (cns_forward did not run)
    _check_all(hip, J, got[0], got[1], want, group)
    assert _same(got, one), "the default path and cns_extend differ"
    if third:
        assert _share_ok2(want) >= 1 / 3


@pytest.mark.parametrize("build", [_control_jobs, _row_of_96_jobs], ids=["identical pairs", "rows of 96 diagonals"])
def test_no_hand_over_without_a_reason(hip, ctx, orc, monkeypatch, build):
    J = build()
    want = J.want(orc, 0.15, 500)
    vol, ja = J.volume(hip, ctx)
    got = _run(hip, ctx, monkeypatch, vol, ja, 0.15, 500)
    one = _run(hip, ctx, monkeypatch, vol, ja, 0.15, 500, MECAT_CNS_KERNEL="1")
    vol.free()
    assert got[2] == 0, "%d units handed over" % got[2]
    _check_all(hip, J, got[0], got[1], want, "control")
    assert _same(got, one)
    assert all(w[2] for w in want)


# ----------------------------------------------------------------------------- 5
@pytest.mark.parametrize("kernel", [None, "1"])
def test_column_cap_at_its_edge(hip, ctx, orc, monkeypatch, kernel):
    rng = np.random.default_rng(512)
    env = {"MECAT_CNS_KERNEL": kernel} if kernel else {}
    g = rng.integers(0, 4, size=812).astype(np.int8)
    J = _Jobs()
    p = J.add_pair(g, g.copy())
    for chain in (0, 1):
        J.add(p, 300, 300, chain)                        # left 300 columns, right exactly 512
        J.add(p, 299, 299, chain)                        # right 513
        J.add(p, 512, 512, chain)                        # left exactly 512, right 300
        J.add(p, 513, 513, chain)                        # left 513
    vol, ja = J.volume(hip, ctx)
    want = J.want(orc, 0.15, 500)
    roomy = _run(hip, ctx, monkeypatch, vol, ja, 0.15, 500, **env)
    _check_all(hip, J, roomy[0], roomy[1], want, "column cap")
    assert [(int(r["left_cols"]), int(r["right_cols"])) for r in roomy[0][:4]] == [(300, 512), (299, 513), (512, 300), (513, 299)]
    for i in range(len(ja)):
        cols = max(int(roomy[0][i]["left_cols"]), int(roomy[0][i]["right_cols"]))
        if cols <= 512:
            res, ops, _ = _run(hip, ctx, monkeypatch, vol, ja[i: i + 1], 0.15, 500, 512, **env)
            assert res[0] == roomy[0][i] and np.array_equal(ops[0], roomy[1][i][:, :32])
        else:
            with pytest.raises(hip.MhipError, match="columns"):
                _run(hip, ctx, monkeypatch, vol, ja[i: i + 1], 0.15, 500, 512, **env)
    vol.free()
