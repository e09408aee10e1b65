"""dw_extend2's snake step with its minimum taken in 16 bits, pass 2's y formed from x - mk_l and a literal, and pass 2's ring reads
requested at the top of a two-pass row (profiles/dw_row_latency.md), against the oracle's DiffAligner restatement and the one-unit kernel
(dw_extend), and the same pairs through cns_forward (dw_extend2<true>) against what test_gpu_cns_forward_edges compares with.
A wrong build shows as wrong coordinates of the units that meet a case, not as a fault: no case here tries to overrun anything.

nn = min(m, limc) is taken as v_min_u16: m is 0 .. 30 (doubled: 0 .. 15 equal bases) or 0x7ffffffe (the whole window of 16 matches), whose
low half 0xfffe is still above any limc; limc (doubled) is 0 .. 32 on a live lane.  So the cases are the values of limc and the two
outcomes of the compare around them.  Pass 2's entries of the row in front are read before pass 1 stores, through the same position
(pb_l): the cases are the rows where that position and the row being written lie far apart (a relocation) or close together.

The pool: identical arms of n bases against n + 1 / n + 23 (n = 1 .. 33, 47, 48, 63, 64: a last block of its own, the shorter side the
query in one job and the target in the other), the same with the last base of the shorter side substituted (the neighbouring diagonal of
the next row then starts on the block's last base: nothing left), against an identical anchor arm; and test_gpu_dw_ring_linear's EVENTS pool
(seed 1123: pairs of 0.9 - 2.8 kb at 10 / 15 / 25 % error, pairs with one insertion of 40 - 100 bases, the TAILS pairs).  The classes are found
on the CPU with test_gpu_dw_scalar_side's restatement of the band rule (`_block`), which gives the furthest x of every diagonal of every row:
where a diagonal starts in a row follows from the row in front (`_starts`), and the snake is the difference.  Classes, each shown by at
least one chosen job (the test prints the counts and asserts that none is zero):

    snake of exactly 16 / 32 bases             a diagonal inside its block runs 16 (32) equal bases and stops at the next one: nn == limc == 32
                                               for one step (two steps in a row), then a step that moves nothing or less than a window
    block end: query / target side, r left     a diagonal that reaches that end of its block starts its snake r = 0, 1, 15, 16, 31 or 32 bases
                                               in front of it: the last step has limc = r mod 16 bases (0 after whole windows, and at once)
    last block of 1 - 31 bases                 the block is shorter than two windows
    pass 2 ends the block at t_len             the end row has 33 - 63 slots and a diagonal of its second pass stands at y == t_len
    pass 2 at t_len - 1 in the end row         ... at y == t_len - 1: one base short of the target's end
    two-pass dual row behind a relocation      a dual row of the two-pass loop (both halves in a block, the wider at 33 - 63) in which a half of
                                               33 slots or more starts at the ring's origin: pass 2's early reads reach the row in front
                                               near the ring's end through pb_l
    dual: one-pass half beside a two-pass half a dual row of the two-pass loop whose narrower half has at most 32 slots: its pass 2 is idle

Per job list: dw_extend2 equals the oracle field by field on the default grid, on four waves and in reverse job order, and equals the
one-unit kernel.  Counter 8, the units handed over, of the chosen list on the default grid is HANDED_OVER, recorded from a run of this
test with the parent commit's library on the same list (MECAT_HIP_LIB): nothing here moves a hand-over."""
import numpy as np
import pytest

import test_gpu_cns_forward_edges as E
import test_gpu_dw_ring_linear as RL
import test_gpu_dw_row_exits as X
import test_gpu_dw_scalar_side as S
from test_gpu_dw_doubled import MIN_ALN
from test_gpu_dw_snake_end import _DwJobs, _join, _run, _same_arm

pytestmark = pytest.mark.gpu

PER_CLASS = 2
HANDED_OVER = 0         # units handed over by the chosen list on the default grid, as the parent commit's library counts them
SHORT = tuple(range(1, 34)) + (47, 48, 63, 64)
RESTS = (0, 1, 15, 16, 31, 32)
CLASSES = (("snake of exactly 16 bases", "snake of exactly 32 bases")
           + tuple("block end: %s side, %d left" % (s, r) for s in ("query", "target") for r in RESTS)
           + ("last block of 1 - 31 bases", "pass 2 ends the block at t_len", "pass 2 at t_len - 1 in the end row",
              "two-pass dual row behind a relocation", "dual: one-pass half beside a two-pass half"))


@pytest.fixture(scope="module")
def hip():
    import mecat_amd.hip as M
    return M


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


# ---- the classes

def _starts(rows, i):
    """where the diagonals of row i start their snake: S._block's rule on the row in front"""
    min_k, x = rows[i][0], rows[i][1]
    if i == 0:
        return np.zeros(1, np.int64)
    pmin, px = rows[i - 1][0], rows[i - 1][1]
    ks = min_k + 2 * np.arange(len(x))
    n = len(px)
    L, R = px[np.clip((ks - 1 - pmin) // 2, 0, n - 1)], px[np.clip((ks + 1 - pmin) // 2, 0, n - 1)]
    x0 = np.where(L < R, R, L + 1)
    x0[-1] = L[-1] + 1
    x0[0] = R[0]
    return x0


def _blocks(q, t):
    """S._direction's block loop -> [(query bases, target bases, last block, rows, end)] of one direction"""
    qidx = tidx = 0
    out = []
    while True:
        ql, tl = len(q) - qidx, len(t) - tidx
        if ql < S.SEG_BLK + 100 or tl < S.SEG_BLK + 100:
            qb, tb, last_block = min(ql, int(tl + tl * 0.2)), min(tl, int(ql + ql * 0.2)), True
        else:
            qb, tb, last_block = S.SEG_BLK, S.SEG_BLK, False
        rows, end = S._block(q[qidx:qidx + qb], t[tidx:tidx + tb])
        out.append((qb, tb, last_block, rows, end))
        if end is None:
            return out
        d, k, x = end
        found, acnt, cx, ck = S._tail(rows, end)
        if not (found and (x + (x - k) + d) // 2 - acnt >= 2) or last_block or not (qb - x <= 20 or tb - (x - k) <= 20):
            return out
        qidx += cx
        tidx += cx - ck


def _classes(case):
    q, t, qs, ts = case[:4]
    got = set()
    units = [_blocks(q[:qs][::-1], t[:ts][::-1]), _blocks(q[qs:], t[ts:])]
    for u in units:
        for qb, tb, last_block, rows, end in u:
            if last_block and 1 <= min(qb, tb) <= 31 and rows:
                got.add("last block of 1 - 31 bases")
            for i, (min_k, x, _, _) in enumerate(rows):
                ks = min_k + 2 * np.arange(len(x))
                x0 = _starts(rows, i)
                y0, y = x0 - ks, x - ks
                run = x - x0
                inside = (x < qb) & (y < tb)
                if (inside & (run == 16)).any():
                    got.add("snake of exactly 16 bases")
                if (inside & (run == 32)).any():
                    got.add("snake of exactly 32 bases")
                if end is None or i + 1 < len(rows):
                    continue
                for j in np.nonzero((x >= qb) | (y >= tb))[0]:                 # the end row: every diagonal that reached an end
                    rq, rt = qb - int(x0[j]), tb - int(y0[j])
                    side, r = ("query", rq) if rq <= rt else ("target", rt)
                    if r in RESTS:
                        got.add("block end: %s side, %d left" % (side, r))
                if 33 <= len(x) <= 63:
                    if (y[32:] == tb).any():
                        got.add("pass 2 ends the block at t_len")
                    if (y[32:] == tb - 1).any():
                        got.add("pass 2 at t_len - 1 in the end row")
    rings = [[RL._ring([len(r[1]) for r in b[3]]) for b in u] for u in units]      # every block's rows in the ring
    for a, b in X._dual_pos(rings):
        if a is None or b is None:
            continue
        na, nb = a[2][2], b[2][2]
        if not 33 <= max(na, nb) <= 63:
            continue
        if (a[2][0] and na >= 33) or (b[2][0] and nb >= 33):
            got.add("two-pass dual row behind a relocation")
        if min(na, nb) <= 32:
            got.add("dual: one-pass half beside a two-pass half")
    return got


# ---- the pool

def _short_pairs():
    """[(q, t, qstart, tstart, chain, meant to align)]: a last block of n bases against n + extra, identical (or but for the last base of the
    shorter side), the anchor on the other side of the seed point; each also with query and target exchanged"""
    rng = np.random.default_rng(5716)
    out = []
    for n in SHORT:
        for extra, subst in ((1, False), (23, False), (2, True)):
            short, long_ = _same_arm(rng, n, n + extra)
            if subst:
                short[-1] = (short[-1] + 1) & 3
            anchor = _same_arm(rng, 560, 560)
            q, t, qs, ts = _join((short, long_), anchor) if n & 1 else _join(anchor, (short, long_))
            chain = (n + extra) & 1
            out.append((q, t, qs, ts, chain, True))
            out.append((t, q, ts, qs, 1 - chain, True))
    return out


def _build_pool():
    cases = _short_pairs() + list(RL._build_events()[0])
    return cases, [_classes(c) for c in cases]


@pytest.fixture(scope="module")
def pool():
    return _build_pool()


@pytest.fixture(scope="module")
def chosen(pool):
    """the jobs that show a class: PER_CLASS of each, the first of the pool"""
    cases, classes = pool
    count = {c: sum(1 for k in classes if c in k) for c in CLASSES}
    print("pool of %d jobs; jobs per class: %s" % (len(cases), count))
    missing = [c for c in CLASSES if not count[c]]
    assert not missing, "no job of the pool shows %s" % missing
    pick = []
    for c in CLASSES:
        pick += [i for i, k in enumerate(classes) if c in k][:PER_CLASS]
    return sorted(set(pick))


def test_chosen_jobs_match_oracle_and_one_unit_kernel(hip, ctx, pool, chosen, monkeypatch):
    cases, classes = pool
    J = _DwJobs([cases[i] for i in chosen])
    n = len(J.jobs)
    lens = [len(cases[i][0]) for i in chosen] + [len(cases[i][1]) for i in chosen]
    print("%d jobs, reads of %d - %d bases, the oracle accepts %d" % (n, min(lens), max(lens), sum(w[0] for w in J.want)))
    missed = [(i, J.jobs[i], J.want[i]) for i in range(n) if cases[chosen[i]][5] and not J.want[i][0]]
    assert not missed, "the oracle rejects %d pairs that are meant to align: %s" % (len(missed), missed[:4])
    gv, wide, narrow, single, cnt = RL._three_ways(hip, ctx, monkeypatch, J)
    print("%d jobs: rows relocated %d, tail-walk steps through a link %d, units handed over %d" % ((n,) + cnt))
    back, _ = _run(hip, ctx, gv, J.jobs[::-1])                            # the job list in its other order
    gv.free()
    RL._compare(J, wide, narrow, single)
    assert back[::-1] == wide, "the results depend on the order of the job list"
    assert cnt[0] > 0, "no row was relocated: the path was not taken"
    assert cnt[2] == HANDED_OVER, "units handed over: %d, the parent commit's library hands over %s" % (cnt[2], HANDED_OVER)


def test_chosen_jobs_in_cns_forward(hip, ctx, pool, chosen, monkeypatch):
    """the same pairs under mecat2cns' block rules: oracle (orc_cns_dw, orc_cns_get_alignment, both aligned strings), cns_extend, four waves"""
    cases = pool[0]
    J = E._Jobs()
    for i in chosen:
        q, t, qs, ts, chain, _ = cases[i]
        J.add_new(q, t, qs, ts, chain)
    assert J.longest() <= 4300
    orc = E._Orc()
    want = J.want(orc, 0.15, MIN_ALN)
    orc.close()
    vol, ja = J.volume(hip, ctx)
    got = E._run(hip, ctx, monkeypatch, vol, ja, 0.15, MIN_ALN)
    cnt = RL._counters(ctx)
    narrow = E._run(hip, ctx, monkeypatch, vol, ja, 0.15, MIN_ALN, MECAT_CNS_WAVES="4")
    one = E._run(hip, ctx, monkeypatch, vol, ja, 0.15, MIN_ALN, MECAT_CNS_KERNEL="1")
    vol.free()
    print("cns_forward: %d jobs, the oracle accepts %.0f %%, rows relocated %d, tail-walk steps through a link %d, units handed over %d"
          % ((len(J), 100 * E._share_ok2(want)) + cnt))
    E._check_all(hip, J, got[0], got[1], want, "snake minimum in 16 bits")
    assert E._same(got, narrow), "the default grid and four waves differ"
    assert E._same(got, one), "the default path and cns_extend differ"
    assert one[2] == 0                                            # (cns_forward did not run)
    assert cnt[0] > 0
