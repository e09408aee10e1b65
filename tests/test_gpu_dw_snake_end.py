"""dw_extend2's snake loop and its idle lanes against the oracle's DiffAligner restatement and the one-unit kernel (dw_extend), and the same
pairs through cns_forward (dw_extend2<true>) against what test_gpu_cns_forward_edges compares with.  The snake step decides with one
compare, nn == min(rest of the query, rest of the target, 16 bases), whether a lane's window or its block ran out, and tells the two apart
only when an active lane has it; idle lanes are not parked and snake on whatever the ring and the staged words give them.  The shapes are
the smallest at which either can go wrong:

* identical pairs with unequal block lengths whose shorter side ends 0, 1, 15, 16, 17, 31, 32 or 33 bases behind a snake step of the main
  diagonal (lengths 16 k + 0, 1, 15 and their neighbours), as a last block of its own, as a last block of 496 + n bases and behind a
  full block; the query the shorter side in one direction and the target in the other, both strands: a whole window that matches with
  nothing behind it (limc == 32 == nn) against a block that ran out (limc < 32);
* staggered lanes: an identical pair with one extra base near the seed point (two diagonals alive) and one substitution 20 - 40 bases in
  front of the end of the shorter sequence: one diagonal ends the block in its first step of a pass while its neighbour needs further ones;
* low-complexity pairs (A homopolymers, (AC)n, (ACG)n; 600 - 1 500 bases; 0, 5 and 15 % substitutions and indels), interleaved with
  random-sequence pairs at 15 %: the idle lanes beside a narrow band see matching bases wherever they look;
* four unrelated pairs (hand-over) and a job at qstart = sstart = 0.

Every job is compared field by field, at the default grid and with four waves (each half runs many units, unlike units share a wave).
The oracle accepts every pair that is meant to align (all but the unrelated ones)."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import test_gpu_cns_forward_edges as E
from test_gpu_dw_doubled import FIELDS, MIN_ALN, _mutate

pytestmark = pytest.mark.gpu

ENDS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65)           # a block of its own, and 496 + n
BEHIND_FULL = (111, 112, 113, 127, 128, 129)                     # 496 + n >= 600: a full block, then a last block of n bases
ANCHOR = 560                                                     # an identical arm that makes a pair long enough to be accepted


@pytest.fixture(scope="module")
def hip():
    import mecat_amd.hip as M
    return M


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


def _join(left, right):
    """(q, t, qstart, tstart) from the two arms (query bases, target bases), each read away from the seed point"""
    (ql, tl), (qr, tr) = left, right
    return np.concatenate([ql[::-1], qr]).astype(np.int8), np.concatenate([tl[::-1], tr]).astype(np.int8), len(ql), len(tl)


def _same_arm(rng, nq, nt):
    g = rng.integers(0, 4, size=max(nq, nt)).astype(np.int8)
    return g[:nq].copy(), g[:nt].copy()


def _build_cases():
    """[(q, t, qstart, tstart, chain, meant to align)]"""
    rng = np.random.default_rng(16032)
    out = []

    def both_ways(q, t, qs, ts, chain, meant=True):
        out.append((q, t, qs, ts, chain, meant))
        out.append((t, q, ts, qs, 1 - chain, meant))

    # 1. identical pairs, unequal block lengths
    for n in ENDS + BEHIND_FULL:
        for extra in (1, 23):
            chain = (n + extra) & 1
            if n in ENDS:
                # the block of n (n + extra) bases on one side of the seed point, the anchor on the other
                edge = _same_arm(rng, n, n + extra)
                both_ways(*_join(edge, _same_arm(rng, ANCHOR, ANCHOR)), chain)
                both_ways(*_join(_same_arm(rng, ANCHOR, ANCHOR), (edge[1], edge[0])), 1 - chain)
            # 496 + n bases: the query the shorter side on the left, the target on the right
            short, long_ = 496 + n, 496 + n + extra
            lq, lt = _same_arm(rng, short, long_)
            rt, rq = _same_arm(rng, short, long_)
            both_ways(*_join((lq, lt), (rq, rt)), chain)
    # 2. staggered lanes
    for it in range(96):
        L = int(rng.integers(120, 700))
        g = rng.integers(0, 4, size=L + 60).astype(np.int8)
        at = int(rng.integers(3, 13))
        short = g[:L].copy()
        s = 20 + (it * 7) % 21
        short[L - s] = (short[L - s] + 1 + it % 3) & 3
        long_ = np.concatenate([g[:at], [(g[at] + 1) & 3], g[at:L + int(rng.integers(0, 40))]]).astype(np.int8)
        arm = (short, long_) if it & 1 else (long_, short)
        anchor = _same_arm(rng, ANCHOR, ANCHOR)
        q, t, qs, ts = _join(arm, anchor) if it & 2 else _join(anchor, arm)
        both_ways(q, t, qs, ts, (it >> 2) & 1)
    # 3. low-complexity pairs between random-sequence pairs
    units = (np.array([0], np.int8), np.array([0, 1], np.int8), np.array([0, 1, 2], np.int8))
    for it in range(54):
        e = (0.0, 0.05, 0.15)[it % 3]
        unit = units[(it // 3) % 3]
        n = int(rng.integers(600, 1500))
        g = np.tile(unit, n // len(unit) + 1)[:n]
        q, t = _mutate(rng, g, e), _mutate(rng, g, e)
        frac = (0.3, 0.5, 0.7)[(it // 9) % 3]
        both_ways(q, t, int(len(q) * frac), int(len(t) * frac), it & 1)
        L = int(rng.integers(1000, 3000))
        g = rng.integers(0, 4, size=L).astype(np.int8)
        cut = int(rng.integers(300, L - 300))
        qp, tp = [_mutate(rng, p, 0.15) for p in np.split(g, [cut])], [_mutate(rng, p, 0.15) for p in np.split(g, [cut])]
        both_ways(np.concatenate(qp), np.concatenate(tp), len(qp[0]), len(tp[0]), (it >> 1) & 1)
    # 4. unrelated pairs (their full blocks reach no end: hand-over); identical reads extended from their first base
    for it in range(4):
        out.append((rng.integers(0, 4, size=2500).astype(np.int8), rng.integers(0, 4, size=2600).astype(np.int8), 1200, 1300, it & 1, False))
    g = rng.integers(0, 4, size=1800).astype(np.int8)
    out.append((g, g.copy(), 0, 0, 0, True))
    return out


@pytest.fixture(scope="module")
def cases():
    return _build_cases()


class _DwJobs:
    """the job list over a volume of its own, with the oracle's answer per job (test_gpu_dw_doubled._Jobs, over given cases)"""

    def __init__(self, cases):
        self.seqs, self.jobs, self.want = [], [], []
        al = H.orc().orc_aligner_new()
        for q, t, qs, ts, chain, _ in cases:
            i = len(self.seqs)
            self.seqs += [(3 - q[::-1]).astype(np.int8) if chain else q, t]          # the volume holds the read as sequenced
            self.jobs.append((i, i + 1, chain, qs, ts))
            q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
            o = H.OrcAlnResult()
            H.orc().orc_dw_go(al, q.ctypes.data, qs, len(q), t.ctypes.data, ts, len(t), MIN_ALN, C.byref(o))
            self.want.append((o.ok, o.query_start, o.query_end, o.target_start, o.target_end, o.matches, o.columns))
        H.orc().orc_aligner_free(al)

    def volume(self, hip, ctx):
        seqs = self.seqs + [np.zeros(64, np.int8)]                        # (no job's read is the last of the volume)
        lens = np.array([len(s) for s in seqs], dtype=np.int32)
        ov = H.orc_pack(np.concatenate(seqs).astype(np.uint8), lens)
        offs, pac = H.vol_arrays(ov)
        return hip.Volume(ctx, pac, offs, ov.contents.num_bases, 0)


def _run(hip, ctx, gv, jobs):
    """-> (results, units dw_extend2 handed over to dw_extend: debug counter 8)"""
    ctx.reset_stats()
    out = hip.align_candidates(ctx, gv, gv, np.array(jobs, dtype=hip.JOB_DTYPE), MIN_ALN)
    return [tuple(int(r[f]) for f in FIELDS) for r in out], ctx.debug_counter(8)


def test_snake_ends_match_oracle_and_one_unit_kernel(hip, ctx, cases, monkeypatch):
    J = _DwJobs(cases)
    n = len(J.jobs)
    meant = [c[5] for c in cases]
    print("%d jobs, %d meant to align, the oracle accepts %d" % (n, sum(meant), sum(w[0] for w in J.want)))
    missed = [(i, J.jobs[i], J.want[i]) for i in range(n) if meant[i] and not J.want[i][0]]
    assert not missed, "the oracle rejects %d pairs that are meant to align: %s" % (len(missed), missed[:4])
    gv = J.volume(hip, ctx)
    monkeypatch.delenv("MECAT_DW_KERNEL", raising=False)
    monkeypatch.delenv("MECAT_DW_WAVES", raising=False)
    wide, handed = _run(hip, ctx, gv, J.jobs)
    monkeypatch.setenv("MECAT_DW_WAVES", "4")
    narrow, _ = _run(hip, ctx, gv, J.jobs)
    monkeypatch.delenv("MECAT_DW_WAVES")
    monkeypatch.setenv("MECAT_DW_KERNEL", "1")
    single, _ = _run(hip, ctx, gv, J.jobs)
    monkeypatch.delenv("MECAT_DW_KERNEL")
    gv.free()
    print("%d units handed over" % handed)
    assert handed >= 4, "the unrelated pairs were not handed over: the path was not taken"
    for what, got in (("dw_extend2", wide), ("dw_extend2 on four waves", narrow)):
        bad = [(i, J.jobs[i], got[i], J.want[i]) for i in range(n) if got[i] != J.want[i]]
        assert not bad, "%s: %d/%d differ from the oracle: %s" % (what, len(bad), n, bad[:4])
    bad = [(i, J.jobs[i], wide[i], single[i]) for i in range(n) if wide[i] != single[i]]
    assert not bad, "dw_extend2 and dw_extend differ on %d/%d: %s" % (len(bad), n, bad[:4])


def test_snake_ends_in_cns_forward(hip, ctx, cases, monkeypatch):
    """the same pairs under mecat2cns' block rules: oracle (orc_cns_dw, orc_cns_get_alignment, both aligned strings), cns_extend, four waves"""
    J = E._Jobs()
    for q, t, qs, ts, chain, _ in cases:
        J.add_new(q, t, qs, ts, chain)
    assert J.longest() <= 4300
    orc = E._Orc()
    want = J.want(orc, 0.15, MIN_ALN)
    orc.close()
    vol, ja = J.volume(hip, ctx)
    got = E._run(hip, ctx, monkeypatch, vol, ja, 0.15, MIN_ALN)
    narrow = E._run(hip, ctx, monkeypatch, vol, ja, 0.15, MIN_ALN, MECAT_CNS_WAVES="4")
    one = E._run(hip, ctx, monkeypatch, vol, ja, 0.15, MIN_ALN, MECAT_CNS_KERNEL="1")
    vol.free()
    print("cns_forward: %d jobs, the oracle accepts %.0f %%, %d units handed over" % (len(J), 100 * E._share_ok2(want), got[2]))
    E._check_all(hip, J, got[0], got[1], want, "snake ends")
    assert E._same(got, narrow), "the default grid and four waves differ"
    assert E._same(got, one), "the default path and cns_extend differ"
    assert one[2] == 0                                            # (cns_forward did not run)
