"""dw_extend2's scalar side — the lane masks of a two-pass row's passes from one s_bfm_b64 per half, the band update's words put together
by moves and its slot counts from one sum, and the one-pass loop's `full` test and the two loops' tests next to them — against the
oracle's DiffAligner restatement and the one-unit kernel (dw_extend), and the same pairs through cns_forward (dw_extend2<true>) against
what test_gpu_cns_forward_edges compares with.  (The classes around 32 slots were chosen for a one-pass loop bound at 31 slots with a
peeled 32-slot row, which was built, passed this test and measured slower, profiles/dw_scalar_side.md; they stay: 32 is where a half's
mask fills its word, where the entry behind a row needs its own store, and where the two loops hand over.)

What the changed code depends on is a row's slot count in each half, so the jobs are chosen by slot counts, on the CPU: `_direction`
restates the band rule in numpy (furthest x per diagonal, qualifying diagonals 2 x - k >= best - band_tol, slots = last - first + 2, the
block rules and the tail walk that places the next block) and gives the slot-count sequence of every block of a pair; its block and cell
counts are compared with the oracle's own counters for every job it follows to the end.  `_dual_rows` lays the two directions of one job
side by side the way the two halves of a wave run them when the job is alone in a launch (both halves pull their unit in the same
instruction and start their first block together; a half between blocks holds the other one up for no row).

The pool (seed 2718, 48 jobs): POOL_15 = 14 pairs of 1 - 3 kb at 15 % error and POOL_30 = 6 at 30 %, POOL_INS = 12 pairs at 5 % with one
insertion of 40 - 90 bases 60 - 400 bases from the seed point, POOL_SHORT = 14 pairs whose one arm is a last block of 1 - 60 bases at 30 %
(band_tol + 1 below 31) against an identical anchor arm, and the two LIMIT_SEEDS cases: a last block of 104 - 260 bases at 45 %, which
runs out of rows with a wide band (no pair of the other groups does; the seeds were found by a search with `_classes`).  The restatement
follows 43 of the 48 to the end of both directions (the others have a block that reaches no end, where the reference goes on from its best
point), and the oracle accepts every pair that is meant to align.  Classes looked for in every block of every unit, and dual classes,
looked for in the dual rows of a job alone in its launch, with the number of pool jobs that show each (the test prints them and asserts
that none is zero):

    at 31 / at 32 / at 33                      a row of exactly that many slots                                        34 / 34 / 34
    31-32-31 / 32-33                           those counts in consecutive rows                                        8 / 34
    32 behind a two-pass row                   a row of 32 slots behind a row of 33 - 63                               17
    32 at the end                              the row that reaches an end of its block has 32 slots                   2
    32 at the row limit                        row max_d - 1 of a block that reaches no end has 32 slots (rows_more 0) 2
    at 62 / at 63 / at 64                      the two-pass bound and the hand-off to the general form                 15 / 14 / 14
    limit below 31 met                         a block with band_tol + 1 < 31 whose band reaches exactly that          3
    words: low half empty / high half empty    a two-pass row whose qualifying diagonals all lie in pass 2's word /    1 / 27
                                               all in pass 1's word (`wa` or `wb` with an empty half)
    dual: 32 beside 1 - 3                      a dual row with 32 slots in one half and 1 - 3 in the other             4
    dual: 32 beside 32                         32 slots in both halves                                                 11
    dual: 32 first behind the two-pass loop    a dual row of at most 32 with a half at 32, behind a two-pass dual row  9
    dual: pass 2 in half a only / b only       a two-pass dual row with 33 or more slots in that half only             20 / 20

(The qualifying diagonals of a row are first .. last, pass 1's word holds slots 0 - 31 and pass 2's 32 - 63: a first diagonal in pass 2's
word puts the last there too.  So the two words of a half are both occupied, or one of them is empty: the two one-sided forms are the
classes.)

The jobs that show a class are run together (default grid, four waves, dw_extend), each dual-class job also alone in a launch of its own
(its two units meet in one wave), and the whole selection alone on one workgroup, where unlike rows pair up in a wave.  The oracle accepts
every pair that is meant to align."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import test_gpu_cns_forward_edges as E
from test_gpu_dw_doubled import FIELDS, MIN_ALN, _mutate
from test_gpu_dw_snake_end import _DwJobs, _join, _run, _same_arm

pytestmark = pytest.mark.gpu

SEG_BLK = 500
POOL_15, POOL_30, POOL_INS, POOL_SHORT = 14, 6, 12, 14
LIMIT_SEEDS = (160, 515)      # _pair_limit cases whose block has 32 slots in its last row before the row limit (found by search)
PER_CLASS = 2                  # jobs taken per class
UNIT_CLASSES = ("at 31", "at 32", "at 33", "31-32-31", "32-33", "32 behind a two-pass row", "32 at the end", "32 at the row limit",
                "at 62", "at 63", "at 64", "limit below 31 met", "words: low half empty", "words: high half empty")
DUAL_CLASSES = ("dual: 32 beside 1 - 3", "dual: 32 beside 32", "dual: 32 first behind the two-pass loop", "dual: pass 2 in half a only",
                "dual: pass 2 in half b only")
CLASSES = UNIT_CLASSES + DUAL_CLASSES


@pytest.fixture(scope="module")
def hip():
    import mecat_amd.hip as M
    return M


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


# ---- the band rule, restated

def _block(Q, T):
    """one block of DiffAligner::Align -> (rows, end): rows = [(min_k, x per diagonal, first, last)] of the rows that ran, first / last the
    qualifying slots of the band update behind the row; end = (d, k, x) of the lowest diagonal that reached an end of the block, or None"""
    qb, tb = len(Q), len(T)
    band_tol, max_d = int(0.3 * max(qb, tb)), int(.3 * (qb + tb))
    qp = np.concatenate([Q, np.full(20, 4, np.int8)])
    tp = np.concatenate([T, np.full(20, 5, np.int8)])
    w = np.arange(16)
    rows, min_k, max_k, best, prev = [], 0, 0, -1, None
    for d in range(max_d):
        if max_k - min_k > 2 * band_tol:
            break
        ks = np.arange(min_k, max_k + 1, 2)
        if prev is None:
            x = np.zeros(1, np.int64)
        else:
            pmin, px = prev
            n = len(px)
            li, ri = (ks - 1 - pmin) // 2, (ks + 1 - pmin) // 2
            L, R = px[np.clip(li, 0, n - 1)], px[np.clip(ri, 0, n - 1)]
            x = np.where(L < R, R, L + 1)
            x[-1] = L[-1] + 1
            x[0] = R[0]
        y = x - ks
        go = np.ones(len(ks), bool)
        while go.any():                                     # the snake, 16 bases at a time
            i = np.nonzero(go)[0]
            xi, yi = np.minimum(x[i], qb), np.minimum(y[i], tb)
            eq = qp[xi[:, None] + w] == tp[yi[:, None] + w]
            run = np.where(eq.all(axis=1), 16, eq.argmin(axis=1))
            x[i] += run
            y[i] += run
            go[i] = run == 16
        done = np.nonzero((x >= qb) | (y >= tb))[0]
        best = max(best, int((x + y).max()))
        q = np.nonzero(x + y >= best - band_tol)[0]
        first, last = int(q[0]), int(q[-1])
        rows.append((min_k, x.copy(), first, last))
        if len(done):
            j = int(done[0])
            return rows, (d, int(ks[j]), int(x[j]))
        prev = (min_k, x)
        min_k, max_k = int(ks[first]) - 1, int(ks[last]) + 1
    return rows, None


def _tail(rows, end):
    """the walk back to the last run of four matches (trim_mismatch_end(.., 4, ..)) -> (found, columns, x, k where the walk stands)"""
    cd, ck, cx = end
    acnt = 0
    while True:
        up = cd > 0
        vl = vr = -1
        if up:
            pmin, px = rows[cd - 1][0], rows[cd - 1][1]
            il, ir = ck - 1 - pmin, ck + 1 - pmin
            if 0 <= il <= 2 * (len(px) - 1):
                vl = int(px[il // 2])
            if 0 <= ir <= 2 * (len(px) - 1):
                vr = int(px[ir // 2])
        x1 = max(vl + 1, vr) if up else 0
        sn = cx - x1
        if sn >= 4:
            return True, acnt + 4, cx - 4, ck
        acnt += sn + (1 if up else 0)
        if not up:
            return False, acnt, 0, ck
        cx = max(vl, vr)
        ck += 1 if vl < vr else -1
        cd -= 1


def _direction(q, t):
    """the blocks of one direction (q, t read away from the seed point) -> ([block], followed to the end of the direction);
    block = {"lim": band_tol + 1, "max_d", "ns": slots of each row that ran, "fl": (first, last) behind each row, "end": its end row or None}"""
    qidx = tidx = 0
    out = []
    while True:
        ql, tl = len(q) - qidx, len(t) - tidx
        if ql < SEG_BLK + 100 or tl < SEG_BLK + 100:
            qb, tb, last_block = min(ql, int(tl + tl * 0.2)), min(tl, int(ql + ql * 0.2)), True
        else:
            qb, tb, last_block = SEG_BLK, SEG_BLK, False
        rows, end = _block(q[qidx:qidx + qb], t[tidx:tidx + tb])
        out.append({"lim": int(0.3 * max(qb, tb)) + 1, "max_d": int(.3 * (qb + tb)), "ns": [len(r[1]) for r in rows],
                    "fl": [(r[2], r[3]) for r in rows], "end": end[0] if end else None,
                    "cells": sum(len(r[1]) for r in rows[:-1]) + ((end[1] - rows[-1][0]) // 2 + 1 if end else len(rows[-1][1])) if rows else 0})
        if end is None:
            return out, not rows                   # no end reached: the reference goes on from its best point, which is not restated
        d, k, x = end
        y = x - k
        found, acnt, cx, ck = _tail(rows, end)
        if not (found and (x + y + d) // 2 - acnt >= 2):
            return out, True
        if last_block or not (qb - x <= 20 or tb - y <= 20):
            return out, True
        qidx += cx
        tidx += cx - ck


def _units(case):
    q, t, qs, ts = case[:4]
    left, lok = _direction(q[:qs][::-1], t[:ts][::-1])
    right, rok = _direction(q[qs:], t[ts:])
    return (left, right), lok and rok


def _dual_rows(left, right):
    """[(slots in half a, slots in half b)] of the dual rows of a job alone in its launch, None for a half that has run out of blocks.  A
    half sets its next block up while the other one waits, so rows pair up by position."""
    pos = [[0, 0], [0, 0]]                          # (block, row) of each half
    units = (left, right)
    out = []
    while True:
        pair = []
        for h in (0, 1):
            b, r = pos[h]
            while b < len(units[h]) and r >= len(units[h][b]["ns"]):
                b, r = b + 1, 0
            pos[h] = [b, r]
            pair.append(units[h][b]["ns"][r] if b < len(units[h]) else None)
        if pair[0] is None and pair[1] is None:
            return out
        out.append(tuple(pair))
        pos[0][1] += 1
        pos[1][1] += 1


def _classes(units):
    """the classes a job shows"""
    got = set()
    for u in units:
        for b in u:
            ns, lim = b["ns"], b["lim"]
            for i, n in enumerate(ns):
                nxt = ns[i + 1] if i + 1 < len(ns) else None
                if n in (31, 32, 33, 62, 63, 64):
                    got.add("at %d" % n)
                if n == 31 and nxt == 32 and i + 2 < len(ns) and ns[i + 2] == 31:
                    got.add("31-32-31")
                if n == 32 and nxt == 33:
                    got.add("32-33")
                if 33 <= n <= 63 and nxt == 32:
                    got.add("32 behind a two-pass row")
                if 33 <= n <= 63:
                    first, last = b["fl"][i]
                    if first >= 32:
                        got.add("words: low half empty")
                    if last < 32:
                        got.add("words: high half empty")
            if ns and ns[-1] == 32 and b["end"] is not None:
                got.add("32 at the end")
            if ns and b["end"] is None and len(ns) == b["max_d"] and ns[-1] == 32:
                got.add("32 at the row limit")
            if lim < 31 and lim in ns:
                got.add("limit below 31 met")
    dual = _dual_rows(*units)
    for i, (a, b) in enumerate(dual):
        if a is None or b is None:
            continue
        if (a == 32 and 1 <= b <= 3) or (b == 32 and 1 <= a <= 3):
            got.add("dual: 32 beside 1 - 3")
        if a == 32 and b == 32:
            got.add("dual: 32 beside 32")
        if max(a, b) == 32 and i and None not in dual[i - 1] and 33 <= max(dual[i - 1]) <= 63:
            got.add("dual: 32 first behind the two-pass loop")
        if 33 <= a <= 63 and b <= 32:
            got.add("dual: pass 2 in half a only")
        if 33 <= b <= 63 and a <= 32:
            got.add("dual: pass 2 in half b only")
    return got


# ---- the pool

def _pair_err(rng, e):
    L = int(rng.integers(1000, 3000))
    g = rng.integers(0, 4, size=L).astype(np.int8)
    cut = int(rng.integers(300, L - 300))
    qp, tp = [_mutate(rng, p, e) for p in np.split(g, [cut])], [_mutate(rng, p, e) for p in np.split(g, [cut])]
    return np.concatenate(qp), np.concatenate(tp), len(qp[0]), len(tp[0])


def _pair_ins(rng, it):
    """one insertion of 40 - 90 bases in the query or the target, 60 - 400 bases behind the seed point on either side (5 % error)"""
    L = int(rng.integers(1400, 2800))
    g = rng.integers(0, 4, size=L).astype(np.int8)
    s = int(rng.integers(500, L - 500))
    at = s + int(rng.integers(60, 400)) * (1 if it & 1 else -1)
    parts = [g[:min(s, at)], g[min(s, at):max(s, at)], g[max(s, at):]]
    qp, tp = [_mutate(rng, p, 0.05) for p in parts], [_mutate(rng, p, 0.05) for p in parts]
    extra = rng.integers(0, 4, size=int(rng.integers(40, 91))).astype(np.int8)
    side = qp if it & 2 else tp
    k = 0 if at < s else 2
    side[k] = np.concatenate([side[k], extra]) if at < s else np.concatenate([extra, side[k]])
    ks = 2 if at < s else 1
    return np.concatenate(qp), np.concatenate(tp), sum(len(p) for p in qp[:ks]), sum(len(p) for p in tp[:ks])


def _pair_short(rng, it):
    """a last block of 1 - 60 bases (band_tol + 1 <= 22) at 30 % error on one side of the seed point, an identical anchor on the other"""
    n = 1 + (it * 7) % 60
    g = rng.integers(0, 4, size=3 * n + 64).astype(np.int8)
    arm = (_mutate(rng, g, 0.30)[:n], _mutate(rng, g, 0.30)[: n + it % 4])
    anchor = _same_arm(rng, 560, 560)
    return _join(arm, anchor) if it & 1 else _join(anchor, arm)


def _pair_limit(seed):
    """a last block of 104 - 260 bases at 45 % error per read on one side of the seed point — it runs out of rows (max_d) with a band of
    32 slots or more —, an identical anchor on the other; one generator per case, so that a case is named by its seed"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(104, 260))
    g = rng.integers(0, 4, size=4 * n).astype(np.int8)
    arm = (_mutate(rng, g, 0.45)[:n], _mutate(rng, g, 0.45)[:n])
    anchor = _same_arm(rng, 560, 560)
    return _join(arm, anchor) if seed & 1 else _join(anchor, arm)


def _build_pool():
    """[(q, t, qstart, tstart, chain, meant to align)], the classes of each, its units' blocks, and whether the restatement followed it to the end"""
    rng = np.random.default_rng(2718)
    cases = [_pair_err(rng, 0.15) + (it & 1, True) for it in range(POOL_15)]
    cases += [_pair_err(rng, 0.30) + (it & 1, False) for it in range(POOL_30)]      # (the oracle accepts few of them: not asked to)
    cases += [_pair_ins(rng, it) + ((it >> 2) & 1, True) for it in range(POOL_INS)]
    cases += [_pair_short(rng, it) + ((it >> 1) & 1, True) for it in range(POOL_SHORT)]
    cases += [_pair_limit(seed) + (seed & 1, True) for seed in LIMIT_SEEDS]
    units, followed = zip(*[_units(c) for c in cases])
    return cases, [_classes(u) for u in units], list(units), list(followed)


@pytest.fixture(scope="module")
def pool():
    return _build_pool()


@pytest.fixture(scope="module")
def chosen(pool):
    """the jobs that show a class: PER_CLASS of each, the first of the pool"""
    cases, classes, _, _ = pool
    count = {c: sum(1 for k in classes if c in k) for c in CLASSES}
    print("pool of %d jobs; jobs per class: %s" % (len(cases), count))
    missing = [c for c in CLASSES if not count[c]]
    assert not missing, "no job of the pool shows %s" % missing
    pick = []
    for c in CLASSES:
        pick += [i for i, k in enumerate(classes) if c in k][:PER_CLASS]
    pick = sorted(set(pick))
    dual = sorted({i for c in DUAL_CLASSES for i in [j for j, k in enumerate(classes) if c in k][:PER_CLASS]})
    return pick, dual


def test_restatement_counts_what_the_oracle_counts(pool):
    """blocks and cells (diagonals visited) of every job the restatement follows to the end, against the oracle's own counters"""
    cases, _, units, followed = pool
    al = H.orc().orc_aligner_new()
    bad, n = [], 0
    for i, (q, t, qs, ts, _, _) in enumerate(cases):
        if not followed[i]:
            continue
        n += 1
        q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
        o = H.OrcAlnResult()
        H.orc().orc_dw_go(al, q.ctypes.data, qs, len(q), t.ctypes.data, ts, len(t), MIN_ALN, C.byref(o))
        nb, nc, nsn = C.c_int64(), C.c_int64(), C.c_int64()
        H.orc().orc_dw_counters(al, C.byref(nb), C.byref(nc), C.byref(nsn))
        mine = (sum(len(u) for u in units[i]), sum(b["cells"] for u in units[i] for b in u))
        if mine != (nb.value, nc.value):
            bad.append((i, mine, (nb.value, nc.value)))
    H.orc().orc_aligner_free(al)
    print("%d of %d jobs followed to the end" % (n, len(cases)))
    assert n >= len(cases) // 2
    assert not bad, "the restatement and the oracle count differently on %d jobs: %s" % (len(bad), bad[:4])


def _against_oracle(what, J, got):
    n = len(J.jobs)
    bad = [(i, J.jobs[i], got[i], J.want[i]) for i in range(n) if got[i] != J.want[i]]
    assert not bad, "%s: %d/%d differ from the oracle: %s" % (what, len(bad), n, bad[:4])


def test_chosen_jobs_match_oracle_and_one_unit_kernel(hip, ctx, pool, chosen, monkeypatch):
    cases = [pool[0][i] for i in chosen[0]]
    J = _DwJobs(cases)
    n = len(J.jobs)
    meant = [c[5] for c in cases]
    print("%d jobs, %d meant to align, the oracle accepts %d" % (n, sum(meant), sum(w[0] for w in J.want)))
    missed = [(i, J.jobs[i], J.want[i]) for i in range(n) if meant[i] and not J.want[i][0]]
    assert not missed, "the oracle rejects %d pairs that are meant to align: %s" % (len(missed), missed[:4])
    gv = J.volume(hip, ctx)
    monkeypatch.delenv("MECAT_DW_KERNEL", raising=False)
    monkeypatch.delenv("MECAT_DW_WAVES", raising=False)
    wide, _ = _run(hip, ctx, gv, J.jobs)
    # every dual-class job alone in a launch: its two units are the two halves of one wave
    alone = {}
    for i in chosen[1]:
        at = chosen[0].index(i)
        alone[at] = _run(hip, ctx, gv, [J.jobs[at]])[0][0]
    monkeypatch.setenv("MECAT_DW_WAVES", "4")
    narrow, _ = _run(hip, ctx, gv, J.jobs)                    # the whole selection alone on one workgroup: unlike rows pair up in a wave
    monkeypatch.delenv("MECAT_DW_WAVES")
    monkeypatch.setenv("MECAT_DW_KERNEL", "1")
    single, _ = _run(hip, ctx, gv, J.jobs)
    monkeypatch.delenv("MECAT_DW_KERNEL")
    gv.free()
    _against_oracle("dw_extend2", J, wide)
    _against_oracle("dw_extend2 on four waves", J, narrow)
    bad = [(at, J.jobs[at], got, J.want[at]) for at, got in alone.items() if got != J.want[at]]
    assert not bad, "alone in a launch: %d/%d differ from the oracle: %s" % (len(bad), len(alone), bad[:4])
    bad = [(i, J.jobs[i], wide[i], single[i]) for i in range(n) if wide[i] != single[i]]
    assert not bad, "dw_extend2 and dw_extend differ on %d/%d: %s" % (len(bad), n, bad[:4])


def test_chosen_jobs_in_cns_forward(hip, ctx, pool, chosen, monkeypatch):
    """the same pairs under mecat2cns' block rules: oracle (orc_cns_dw, orc_cns_get_alignment, both aligned strings), cns_extend, four waves"""
    J = E._Jobs()
    for i in chosen[0]:
        q, t, qs, ts, chain, _ = pool[0][i]
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
    E._check_all(hip, J, got[0], got[1], want, "scalar side")
    assert E._same(got, narrow), "the default grid and four waves differ"
    assert E._same(got, one), "the default path and cns_extend differ"
    assert one[2] == 0                                            # (cns_forward did not run)
