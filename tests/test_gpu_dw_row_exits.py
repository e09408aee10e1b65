"""dw_extend2 around its two fast d-row loops — the entry behind a one-pass row, which every lane stores one slot to its right in front
of its own store, so that the row of exactly 32 slots needs no test, and the ways out of the loops when a half's next row would not fit
in front of the ring's end, which come right behind that store (profiles/dw_row_exits.md) — against the oracle's DiffAligner
restatement and the one-unit kernel (dw_extend), and the same pairs through cns_forward (dw_extend2<true>) against what
test_gpu_cns_forward_edges compares with.
A wrong build shows as wrong coordinates of the units that meet a case, not as a fault: no case here tries to overrun the ring.

The pool is test_gpu_dw_ring_linear's EVENTS pool (seed 1123, the same generators: pairs of 0.9 - 2.8 kb at 10 / 15 / 25 % error, pairs
with one insertion of 40 - 100 bases, the TAILS pairs).  What the kernel does here depends only on the slot counts of a unit's rows, so
the classes are found on the CPU: test_gpu_dw_scalar_side's restatement of the band rule (`_units`), test_gpu_dw_ring_linear's layout of a
block's rows in the ring (`_ring`), and the pairing of the two halves' rows of a job that is alone in its launch (`_dual_pos`).  A dual
row runs in the one-pass loop when both halves are in a block and neither has more than 32 slots, in the two-pass loop when the wider has
33 .. 63.  A half `wraps` behind a row when the position behind it is more than 2 048 - 130 bytes into the ring.  Classes, each shown by at
least one chosen job (the test prints the counts and asserts that none of the required ones is zero):

the entry behind a one-pass row
    end row of 32 slots                        the row that reaches an end of its block has 32 slots: the tail walk's first read is the entry
                                               behind it
    32 slots under the tail walk               a TAILS pair whose tail walk steps back over a row of 32 slots (`_walk_back`)
    32 slots in front of a relocation          the row behind a row of 32 slots starts at the ring's origin: the entry behind the 32-slot row
                                               is what the relocation copies to entry 2
    relocated row of 32 slots
    32 slots, then a row cut on the left       the band update behind the row that follows a 32-slot row drops diagonals on the left
    dual: 32 beside 32 / beside a narrower     a dual row of the one-pass loop with both halves at 32 / one at 32 and the other below

the ways out of the fast loops (dual rows of a job alone in its launch, both halves going on in their blocks)
    exit: one-pass loop to a one-pass row / to a two-pass row, two-pass loop to a two-pass row / to a row of 64 slots or more
                                               a half wraps behind a dual row of that loop, and the next dual row is of that kind
    exit: both halves wrap / one half wraps    in the same dual row
    wrap in the end row                        a half wraps behind the row that reaches an end of its block, in a fast loop: no relocation
    wrap in the last row of max_d / in front of the band limit
                                               the same for a block that runs out of rows / whose next row would exceed its band limit;
                                               not required: the test says whether the pool shows them

Per job list: dw_extend2 equals the oracle field by field on the default grid, on four waves and in reverse job order, and equals the
one-unit kernel.  Every chosen job alone in its launch that the restatement follows to its end and that is not handed over: counter 30
(rows relocated) is what `_ring` predicts — a half is relocated exactly when it was — and counter 4 (cells) the sum of its rows' slots.
Counter 8, the units handed over, of the chosen list on the default grid is HANDED_OVER, recorded from a run of the parent commit's
library on the same list (MECAT_HIP_LIB): nothing here moves a hand-over."""
import numpy as np
import pytest

import test_gpu_cns_forward_edges as E
import test_gpu_dw_ring_linear as RL
import test_gpu_dw_scalar_side as S
from test_gpu_dw_doubled import MIN_ALN
from test_gpu_dw_snake_end import _DwJobs, _run

pytestmark = pytest.mark.gpu

PER_CLASS = 2
RING, ROW_STORE = RL.RING, RL.ROW_STORE
HANDED_OVER = 2         # units handed over by the chosen list on the default grid, as the parent commit's library counts them
ENTRY_CLASSES = ("end row of 32 slots", "32 slots under the tail walk", "32 slots in front of a relocation", "relocated row of 32 slots",
                 "32 slots, then a row cut on the left", "dual: 32 beside 32", "dual: 32 beside a narrower half")
EXIT_CLASSES = ("exit: one-pass loop to a one-pass row", "exit: one-pass loop to a two-pass row", "exit: two-pass loop to a two-pass row",
                "exit: two-pass loop to a row of 64 slots or more", "exit: both halves wrap", "exit: one half wraps", "wrap in the end row")
OPTIONAL_CLASSES = ("wrap in the last row of max_d", "wrap in front of the band limit")
CLASSES = ENTRY_CLASSES + EXIT_CLASSES


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

def _wraps(pos):
    """a row of one or two passes at ring byte `pos` would store beyond the ring's end (the kernel's lin_l > wrap_l)"""
    return pos + ROW_STORE + 2 > RING


def _dual_pos(rings):
    """test_gpu_dw_ring_linear._dual with the place of each row: [(entry of half a, entry of half b)], entry = (block, row, `_ring` row) or
    None for a half that has run out of blocks"""
    pos, out = [[0, 0], [0, 0]], []
    while True:
        pair = []
        for h in (0, 1):
            b, r = pos[h]
            while b < len(rings[h]) and r >= len(rings[h][b]):
                b, r = b + 1, 0
            pos[h] = [b, r]
            pair.append((b, r, rings[h][b][r]) if b < len(rings[h]) else None)
        if pair[0] is None and pair[1] is None:
            return out
        out.append(tuple(pair))
        pos[0][1] += 1
        pos[1][1] += 1


def _walk_back(case):
    """the slot counts of the rows that a tail walk of this pair steps back over (S._direction's block loop with S._tail's walk, counting)"""
    q, t, qs, ts = case[:4]
    seen = []
    for qq, tt in ((q[:qs][::-1], t[:ts][::-1]), (q[qs:], t[ts:])):
        qidx = tidx = 0
        while True:
            ql, tl = len(qq) - qidx, len(tt) - tidx
            if ql < S.SEG_BLK + 100 or tl < S.SEG_BLK + 100:
                qb, tb, last_block = min(ql, int(tl + tl * 0.2)), min(tl, int(ql + ql * 0.2)), True
            else:
                qb, tb, last_block = S.SEG_BLK, S.SEG_BLK, False
            rows, end = S._block(qq[qidx:qidx + qb], tt[tidx:tidx + tb])
            if end is None:
                break
            cd, ck, cx = end
            while cd > 0:                                      # S._tail, keeping the rows it leaves behind
                pmin, px = rows[cd - 1][0], rows[cd - 1][1]
                il, ir = ck - 1 - pmin, ck + 1 - pmin
                vl = int(px[il // 2]) if 0 <= il <= 2 * (len(px) - 1) else -1
                vr = int(px[ir // 2]) if 0 <= ir <= 2 * (len(px) - 1) else -1
                if cx - max(vl + 1, vr) >= 4:
                    break
                cx, ck, cd = max(vl, vr), ck + (1 if vl < vr else -1), cd - 1
                seen.append(len(rows[cd][1]))
            d, k, x = end
            found, acnt, wx, wk = S._tail(rows, end)
            if not (found and (x + (x - k) + d) // 2 - acnt >= 2) or last_block or not (qb - x <= 20 or tb - (x - k) <= 20):
                break
            qidx += wx
            tidx += wx - wk
    return seen


def _classes(case, units, is_tail):
    got = set()
    rings = [[RL._ring(b["ns"]) for b in u] for u in units]
    for u, ur in zip(units, rings):
        for b, rows in zip(u, ur):
            for i, (rel, start, n, flat) in enumerate(rows):
                if n != 32:
                    continue
                if rel:
                    got.add("relocated row of 32 slots")
                if i + 1 < len(rows) and rows[i + 1][0]:
                    got.add("32 slots in front of a relocation")
                if i + 1 < len(rows) and b["fl"][i + 1][0] > 0:
                    got.add("32 slots, then a row cut on the left")
                if i + 1 == len(rows) and b["end"] is not None:
                    got.add("end row of 32 slots")
    if is_tail and any(32 in b["ns"][-64:] for u in units for b in u) and 32 in _walk_back(case):
        got.add("32 slots under the tail walk")
    dual = _dual_pos(rings)
    for i, (a, b) in enumerate(dual):
        if a is None or b is None:
            continue                                           # one half alone: the general row form
        na, nb = a[2][2], b[2][2]
        loop = 1 if max(na, nb) <= 32 else 2 if max(na, nb) <= 63 else 0
        if not loop:
            continue
        if na == 32 and nb == 32:
            got.add("dual: 32 beside 32")
        if (na == 32 and nb < 32) or (nb == 32 and na < 32):
            got.add("dual: 32 beside a narrower half")
        behind = [e[2][1] + 2 * e[2][2] + 2 for e in (a, b)]  # the ring position behind each half's row
        last = [e[1] + 1 == len(units[h][e[0]]["ns"]) for h, e in enumerate((a, b))]
        for h, e in enumerate((a, b)):
            if last[h] and _wraps(behind[h]):
                blk = units[h][e[0]]
                got.add("wrap in the end row" if blk["end"] is not None else
                        "wrap in the last row of max_d" if len(blk["ns"]) == blk["max_d"] else "wrap in front of the band limit")
        if last[0] or last[1] or i + 1 >= len(dual) or None in dual[i + 1]:
            continue
        w = [_wraps(p) for p in behind]
        if not (w[0] or w[1]):
            continue
        nxt = max(dual[i + 1][0][2][2], dual[i + 1][1][2][2])
        got.add("exit: %s loop to %s" % (("one-pass", "two-pass")[loop - 1],
                                         "a one-pass row" if nxt <= 32 else "a two-pass row" if nxt <= 63 else "a row of 64 slots or more"))
        got.add("exit: both halves wrap" if w[0] and w[1] else "exit: one half wraps")
    return got


def _build_pool():
    """test_gpu_dw_ring_linear._build_events' cases (same seed, same order) -> (cases, classes of each, (relocations, cells) that `_ring`
    predicts, followed to the end of both directions)"""
    rng = np.random.default_rng(1123)
    cases = []
    for it in range(RL.EV_ERR):
        e = (0.10, 0.15, 0.25)[it % 3]
        cases += [c + ((it + k) & 1, e < 0.2) for k, c in enumerate(RL._swept(rng, e, it))][:2]
    cases += [RL._with_insertion(rng, it) + ((it >> 2) & 1, True) for it in range(RL.EV_INS)]
    first_tail = len(cases)
    cases += [RL._tail_pair(rng, w, it) + ((it >> 3) & 1, True) for w in RL.TAILS for it in range(8)]
    classes, predicted, followed = [], [], []
    for i, c in enumerate(cases):
        units, ok = S._units(c)
        _, nrel, ncell = RL._events(units)
        classes.append(_classes(c, units, i >= first_tail))
        predicted.append((nrel, ncell))
        followed.append(ok)
    return cases, classes, predicted, followed


@pytest.fixture(scope="module")
def pool():
    return _build_pool()


@pytest.fixture(scope="module")
def chosen(pool):
    """the jobs that show a class: PER_CLASS of each, the first of the pool"""
    cases, classes, _, _ = pool
    count = {c: sum(1 for k in classes if c in k) for c in CLASSES + OPTIONAL_CLASSES}
    print("pool of %d jobs; jobs per class: %s" % (len(cases), count))
    missing = [c for c in CLASSES if not count[c]]
    assert not missing, "no job of the pool shows %s" % missing
    print("the pool shows %s" % ", ".join("%s: %s" % (c, "yes" if count[c] else "no") for c in OPTIONAL_CLASSES))
    pick = []
    for c in CLASSES + OPTIONAL_CLASSES:
        pick += [i for i, k in enumerate(classes) if c in k][:PER_CLASS]
    return sorted(set(pick))


def test_chosen_jobs_match_oracle_and_one_unit_kernel(hip, ctx, pool, chosen, monkeypatch):
    cases, classes, predicted, followed = pool
    J = _DwJobs([cases[i] for i in chosen])
    n = len(J.jobs)
    missed = [(i, J.jobs[i], J.want[i]) for i in range(n) if cases[chosen[i]][5] and not J.want[i][0]]
    assert not missed, "the oracle rejects %d pairs that are meant to align: %s" % (len(missed), missed[:4])
    gv, wide, narrow, single, cnt = RL._three_ways(hip, ctx, monkeypatch, J)
    print("%d jobs: rows relocated %d, tail-walk steps through a link %d, units handed over %d" % ((n,) + cnt))
    back, _ = _run(hip, ctx, gv, J.jobs[::-1])                            # the job list in its other order
    alone, exact = {}, []
    for k, i in enumerate(chosen):                                        # alone in a launch: the job's two units are the two halves of one wave
        alone[k] = _run(hip, ctx, gv, [J.jobs[k]])[0][0]
        got = RL._counters(ctx)
        if followed[i] and got[2] == 0:
            exact.append((i, (got[0], ctx.debug_counter(4)), predicted[i]))
    gv.free()
    RL._compare(J, wide, narrow, single)
    assert back[::-1] == wide, "the results depend on the order of the job list"
    bad = [(k, J.jobs[k], got, J.want[k]) for k, got in alone.items() if got != J.want[k]]
    assert not bad, "alone in a launch: %d/%d differ from the oracle: %s" % (len(bad), len(alone), bad[:4])
    print("(relocations, cells), kernel against restatement, of %d jobs alone in a launch: %s" % (len(exact), exact[:8]))
    shown = set().union(*[classes[i] for i, _, _ in exact]) if exact else set()
    unseen = [c for c in CLASSES if c not in shown]
    assert not unseen, "no job with exact counters shows %s" % unseen
    off = [x for x in exact if x[1] != x[2]]
    assert not off, "counter 30 (relocations) or counter 4 (cells) is not what the restatement predicts: %s" % off[:6]
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
    E._check_all(hip, J, got[0], got[1], want, "row exits")
    assert E._same(got, narrow), "the default grid and four waves differ"
    assert E._same(got, one), "the default path and cns_extend differ"
    assert one[2] == 0                                            # (cns_forward did not run)
    assert cnt[0] > 0

