"""dw_extend2's ring of d-rows at linear LDS addresses — a row never straddles the ring's end; the rare row that would is relocated to the
ring's origin, where three reserved entries link it to the row in front — against the oracle's DiffAligner restatement and the one-unit
kernel (dw_extend), which keeps every row, and the same pairs through cns_forward (dw_extend2<true>) against what
test_gpu_cns_forward_edges compares with.  A wrong build shows as wrong coordinates of the units that meet an event, not as a fault: no
case here tries to overrun the ring.

Two job lists.

BULK (seed 4711): BULK_PAIRS pairs of 0.9 - 2.8 kb at 10 / 15 / 25 % error, each with SWEEP seed points 3 - 40 bases apart at corresponding
places, arms of 300 - 1 600 bases and unequal lengths (one read loses up to half of an end), strands alternating: about 2 700 units.
The sweep parameter is the seed point: moving it changes both arms' first blocks and with them the byte at which every later row
starts in the ring.  Compared field by field with the oracle, on the default grid, on four waves and with the one-unit kernel.

EVENTS (seed 1123): what the ring does depends only on the slot counts of a unit's rows, so the events are looked for on the CPU with
test_gpu_dw_scalar_side's restatement of the band rule (`_units`) and `_ring`, which lays a block's rows out the way the kernel does — a
row of ns slots starts at byte 12 of the ring, or 2 ns + 2 bytes behind the row in front, or at byte 6 when
start + max(128, 2 ns) + 2 > 2 048.  The pool is EV_ERR pairs like BULK's, EV_INS pairs with one insertion of 40 - 100 bases (bands of 64
slots and more) and the TAILS pairs: an arm at 15 % error whose last 40 - 120 bases in front of an end of the block — the end of both
reads, or about base 500 of a full block — carry a substitution at every second base behind 24 identical ones, so that the tail walk finds
no run of four matches there and goes back row by row, 20 to 60 rows, from wherever the rows in front left the write point.  Classes, each shown by at least one job (the test prints the counts and asserts that none is zero):

    relocation in front of a one-pass row / a row of 32 slots / a two-pass row / a row of 64 slots or more
    the row that reaches the end of its block is a relocated row
    a row of 64 slots or more that starts, or would have started, within 304 bytes of the ring's end
    dual: both halves relocate in front of the same dual row / one half alone        (a job alone in its launch, rows paired by `_dual`)

and by the kernel's own counters (30: rows relocated, 31: tail-walk steps taken through a link, 8: units handed over):

    every job that the restatement follows to its end, alone in a launch and not handed over: counter 30 is exactly what `_ring` predicts,
    and counter 4, the cells — counted from the ring address plus what the relocations skipped — is the sum of the rows' slots
    the TAILS pairs: counter 31 > 0, and counter 8 > 0 — every block of theirs reaches an end, so a hand-over is a walk that met a row the
    ring no longer holds (it went round twice, or the write point had come within 128 bytes of the row)

The chosen jobs run together, in reverse order, on four waves, each dual-class job alone, and through the one-unit kernel."""
import numpy as np
import pytest

import test_gpu_cns_forward_edges as E
import test_gpu_dw_scalar_side as S
from test_gpu_dw_doubled import MIN_ALN, _mutate
from test_gpu_dw_snake_end import _DwJobs, _join, _run, _same_arm

pytestmark = pytest.mark.gpu

BULK_PAIRS, SWEEP = 270, 5
EV_ERR, EV_INS = 24, 16
TAILS = tuple(range(40, 121, 8))
PER_CLASS = 2
RING, ROW_STORE, ORG, ROW0 = 2048, 128, 6, 12
UNIT_CLASSES = ("relocation: one-pass row next", "relocation: 32 slots next", "relocation: two-pass row next", "relocation: 64 slots or more next",
                "end row at the origin", "64 slots or more within 304 bytes of the end")
DUAL_CLASSES = ("dual: both halves relocate", "dual: one half relocates")
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


# ---- the ring, restated

def _ring(ns):
    """the rows of one block -> [(relocated, start byte, slots, start byte had it not been relocated)]"""
    off, out = ROW0, []
    for n in ns:
        rel = off + max(ROW_STORE, 2 * n) + 2 > RING
        out.append((rel, ORG if rel else off, n, off))
        off = (ORG if rel else off) + 2 * n + 2
    return out


def _dual(rings):
    """[(row of half a, row of half b)] of a job alone in its launch, None for a half that has run out of blocks
    (test_gpu_dw_scalar_side._dual_rows over `_ring` rows)"""
    pos, out = [[0, 0], [0, 0]], []
    while True:
        pair = []
        for h in (0, 1):
            b, r = pos[h]
            while b < len(rings[h]) and r >= len(rings[h][b]):
                b, r = b + 1, 0
            pos[h] = [b, r]
            pair.append(rings[h][b][r] if b < len(rings[h]) else None)
        if pair[0] is None and pair[1] is None:
            return out
        out.append(tuple(pair))
        pos[0][1] += 1
        pos[1][1] += 1


def _events(units):
    """(classes a job shows, relocations of its two units, their cells as the kernel counts them: every slot of every row)"""
    got, nrel = set(), 0
    ncell = sum(n for u in units for b in u for n in b["ns"])
    rings = [[_ring(b["ns"]) for b in u] for u in units]
    for u, ur in zip(units, rings):
        for b, rows in zip(u, ur):
            for rel, start, n, flat in rows:
                nrel += rel
                if rel:
                    got.add("relocation: one-pass row next" if n < 32 else "relocation: 32 slots next" if n == 32 else
                            "relocation: two-pass row next" if n < 64 else "relocation: 64 slots or more next")
                if n >= 64 and RING - flat <= 304:
                    got.add("64 slots or more within 304 bytes of the end")
            if rows and b["end"] is not None and rows[-1][0]:
                got.add("end row at the origin")
    for a, b in _dual(rings):
        if a is not None and b is not None and (a[0] or b[0]):
            got.add("dual: both halves relocate" if a[0] and b[0] else "dual: one half relocates")
    return got, nrel, ncell


# ---- the pairs

def _swept(rng, e, it):
    """[(q, t, qstart, tstart)]: one pair, SWEEP seed points 3 - 40 bases apart"""
    L = int(rng.integers(900, 2800))
    g = rng.integers(0, 4, size=L).astype(np.int8)
    c0 = int(rng.integers(max(300, L - 1800), min(1500, L - 300 - 40 * SWEEP)))
    cuts = c0 + np.cumsum(rng.integers(3, 41, size=SWEEP))
    qp = [_mutate(rng, p, e) for p in np.split(g, cuts)]
    tp = [_mutate(rng, p, e) for p in np.split(g, cuts)]
    if it % 3 == 0:
        tp[-1] = tp[-1][: max(300, len(tp[-1]) - int(rng.integers(0, len(tp[-1]) // 2 + 1)))]      # unequal lengths: an end of one read is missing
    if it % 3 == 1:
        qp[0] = qp[0][max(0, min(len(qp[0]) - 300, int(rng.integers(0, len(qp[0]) // 2 + 1)))):]
    q, t = np.concatenate(qp), np.concatenate(tp)
    return [(q, t, sum(len(p) for p in qp[:k]), sum(len(p) for p in tp[:k])) for k in range(1, SWEEP + 1)]


def _with_insertion(rng, it):
    """one insertion of 40 - 100 bases, 60 - 400 bases from the seed point on either side, 5 % error (test_gpu_dw_scalar_side._pair_ins, wider)"""
    L = int(rng.integers(1400, 2800))
    g = rng.integers(0, 4, size=L).astype(np.int8)
    s = int(rng.integers(500, L - 500))
    at = s + int(rng.integers(60, 400)) * (1 if it & 1 else -1)
    parts = [g[:min(s, at)], g[min(s, at):max(s, at)], g[max(s, at):]]
    qp, tp = [_mutate(rng, p, 0.05) for p in parts], [_mutate(rng, p, 0.05) for p in parts]
    extra = rng.integers(0, 4, size=int(rng.integers(40, 101))).astype(np.int8)
    side = qp if it & 2 else tp
    k = 0 if at < s else 2
    side[k] = np.concatenate([side[k], extra]) if at < s else np.concatenate([extra, side[k]])
    ks = 2 if at < s else 1
    return np.concatenate(qp), np.concatenate(tp), sum(len(p) for p in qp[:ks]), sum(len(p) for p in tp[:ks])


def _tail_pair(rng, width, it):
    """an arm of 250 - 470 bases at 15 % error (its rows take the ring round a few times), 24 identical bases, then a substitution at every
    second base over `width` bases at an end of the block — the end of both reads, or about base 500 of a full block (the arm goes on for
    400 - 700 identical bases) —, and an identical anchor arm on the other side"""
    full = (it >> 1) & 1
    pre = rng.integers(0, 4, size=(500 - 24 - width // 2) if full else int(rng.integers(250, 330))).astype(np.int8)
    rest = rng.integers(0, 4, size=24 + width + (int(rng.integers(400, 700)) if full else 0)).astype(np.int8)
    sub = rest.copy()
    at = np.arange(24, 24 + width, 2)
    sub[at] = (sub[at] + 1 + rng.integers(0, 3, size=len(at))) & 3
    q, t = np.concatenate([_mutate(rng, pre, 0.15), rest]), np.concatenate([_mutate(rng, pre, 0.15), sub])
    arm = (q, t) if it & 4 else (t, q)
    anchor = _same_arm(rng, 560, 560)
    return _join(arm, anchor) if it & 1 else _join(anchor, arm)


def _build_bulk():
    rng = np.random.default_rng(4711)
    cases = []
    for it in range(BULK_PAIRS):
        e = (0.10, 0.15, 0.25)[it % 3]
        cases += [c + ((it + k) & 1, e < 0.2) for k, c in enumerate(_swept(rng, e, it))]
    return cases


def _build_events():
    """[(q, t, qstart, tstart, chain, meant to align)], the classes and predicted relocations of each, whether the restatement followed it to
    the end of both directions, and the indices of the TAILS pairs; relocations come as (relocations, cells)"""
    rng = np.random.default_rng(1123)
    cases = []
    for it in range(EV_ERR):
        e = (0.10, 0.15, 0.25)[it % 3]
        cases += [c + ((it + k) & 1, e < 0.2) for k, c in enumerate(_swept(rng, e, it))][:2]
    cases += [_with_insertion(rng, it) + ((it >> 2) & 1, True) for it in range(EV_INS)]
    tails = list(range(len(cases), len(cases) + 8 * len(TAILS)))
    cases += [_tail_pair(rng, w, it) + ((it >> 3) & 1, True) for w in TAILS for it in range(8)]
    ev, nrel, followed = [], [], []
    for c in cases:
        units, ok = S._units(c)
        e, n, nc = _events(units)
        ev.append(e)
        nrel.append((n, nc))
        followed.append(ok)
    return cases, ev, nrel, followed, tails


@pytest.fixture(scope="module")
def events():
    return _build_events()


@pytest.fixture(scope="module")
def chosen(events):
    """the jobs that show a class (PER_CLASS of each, the first of the pool) and every TAILS pair; the dual-class jobs among them"""
    cases, ev, _, _, tails = events
    count = {c: sum(1 for k in ev if c in k) for c in CLASSES}
    print("pool of %d jobs; jobs per class: %s" % (len(cases), count))
    missing = [c for c in CLASSES if not count[c]]
    assert not missing, "no job of the pool shows %s" % missing
    pick = list(tails)
    for c in CLASSES:
        pick += [i for i, k in enumerate(ev) if c in k][:PER_CLASS]
    dual = sorted({i for c in DUAL_CLASSES for i in [j for j, k in enumerate(ev) if c in k][:PER_CLASS]})
    return sorted(set(pick)), dual


def _counters(ctx):
    """(rows relocated, tail-walk steps through a link, units handed over)"""
    return ctx.debug_counter(30), ctx.debug_counter(31), ctx.debug_counter(8)


def _three_ways(hip, ctx, monkeypatch, J):
    """-> (default grid, four waves, one-unit kernel, (relocations, link steps, handed over) of the default grid)"""
    gv = J.volume(hip, ctx)
    monkeypatch.delenv("MECAT_DW_KERNEL", raising=False)
    monkeypatch.delenv("MECAT_DW_WAVES", raising=False)
    wide, _ = _run(hip, ctx, gv, J.jobs)
    cnt = _counters(ctx)
    monkeypatch.setenv("MECAT_DW_WAVES", "4")
    narrow, _ = _run(hip, ctx, gv, J.jobs)
    monkeypatch.delenv("MECAT_DW_WAVES")
    monkeypatch.setenv("MECAT_DW_KERNEL", "1")
    single, _ = _run(hip, ctx, gv, J.jobs)
    monkeypatch.delenv("MECAT_DW_KERNEL")
    return gv, wide, narrow, single, cnt


def _compare(J, wide, narrow, single):
    n = len(J.jobs)
    for what, got in (("dw_extend2", wide), ("dw_extend2 on four waves", narrow)):
        bad = [(i, J.jobs[i], got[i], J.want[i]) for i in range(n) if got[i] != J.want[i]]
        assert not bad, "%s: %d/%d differ from the oracle: %s" % (what, len(bad), n, bad[:4])
    bad = [(i, J.jobs[i], wide[i], single[i]) for i in range(n) if wide[i] != single[i]]
    assert not bad, "dw_extend2 and dw_extend differ on %d/%d: %s" % (len(bad), n, bad[:4])


def test_bulk_matches_oracle_and_one_unit_kernel(hip, ctx, monkeypatch):
    cases = _build_bulk()
    J = _DwJobs(cases)
    n = len(J.jobs)
    meant = sum(c[5] for c in cases)
    accepted = sum(w[0] for w in J.want)
    print("%d jobs (%d units), %d at 10 or 15 %%, the oracle accepts %d" % (n, 2 * n, meant, accepted))
    assert 2 * n >= 2500 and accepted >= meant // 2
    gv, wide, narrow, single, (nrel, nlink, handed) = _three_ways(hip, ctx, monkeypatch, J)
    gv.free()
    print("rows relocated %d, tail-walk steps through a link %d, units handed over %d" % (nrel, nlink, handed))
    _compare(J, wide, narrow, single)
    assert nrel >= 2 * n, "fewer relocations than units: the rings did not go round"
    assert nlink > 0


def test_events_match_oracle_and_one_unit_kernel(hip, ctx, events, chosen, monkeypatch):
    cases, ev, nrel, followed, tails = events
    pick, dual = chosen
    J = _DwJobs([cases[i] for i in pick])
    n = len(J.jobs)
    missed = [(i, J.jobs[i], J.want[i]) for i in range(n) if cases[pick[i]][5] and not J.want[i][0]]
    assert not missed, "the oracle rejects %d pairs that are meant to align: %s" % (len(missed), missed[:4])
    gv, wide, narrow, single, cnt = _three_ways(hip, ctx, monkeypatch, J)
    print("%d jobs: rows relocated %d, tail-walk steps through a link %d, units handed over %d" % ((n,) + cnt))
    back, _ = _run(hip, ctx, gv, J.jobs[::-1])                            # the job list in its other order
    # the TAILS pairs on their own: every block of theirs reaches an end, so what is handed over is a walk that lost its row
    at = [pick.index(i) for i in tails]
    assert all(followed[i] for i in tails), "a TAILS pair has a block that reaches no end"
    _, _ = _run(hip, ctx, gv, [J.jobs[k] for k in at])
    tail_cnt = _counters(ctx)
    print("%d TAILS jobs: rows relocated %d, tail-walk steps through a link %d, units handed over %d" % ((len(at),) + tail_cnt))
    # every job that was followed to its end, alone in a launch: its two units are the two halves of one wave
    alone, exact = {}, []
    for i in sorted(set(dual) | {j for j in pick if followed[j] and j not in tails}):
        k = pick.index(i)
        alone[k] = _run(hip, ctx, gv, [J.jobs[k]])[0][0]
        got = _counters(ctx)
        if followed[i] and got[2] == 0:
            exact.append((i, (got[0], ctx.debug_counter(4)), nrel[i]))
    gv.free()
    _compare(J, wide, narrow, single)
    assert back[::-1] == wide, "the results depend on the order of the job list"
    bad = [(k, J.jobs[k], got, J.want[k]) for k, got in alone.items() if got != J.want[k]]
    assert not bad, "alone in a launch: %d/%d differ from the oracle: %s" % (len(bad), len(alone), bad[:4])
    print("(relocations, cells), kernel against restatement, of %d jobs alone in a launch: %s" % (len(exact), exact[:8]))
    assert len(exact) >= len(CLASSES)
    off = [x for x in exact if x[1] != x[2]]
    assert not off, "counter 30 (relocations) or counter 4 (cells: the skew of the relocations) is not what the restatement predicts: %s" % off[:6]
    assert tail_cnt[1] > 0, "no tail walk went through a link"
    assert tail_cnt[2] > 0, "no tail walk lost its row: the hand-over was not taken"
    assert tail_cnt[2] < 2 * len(at), "every TAILS unit was handed over: no walk of theirs was finished through a link"


def test_events_in_cns_forward(hip, ctx, events, chosen, monkeypatch):
    """the same pairs under mecat2cns' block rules: oracle (orc_cns_dw, orc_cns_get_alignment, both aligned strings), cns_extend, four waves"""
    cases = events[0]
    J = E._Jobs()
    for i in chosen[0]:
        q, t, qs, ts, chain, _ = cases[i]
        J.add_new(q, t, qs, ts, chain)
    assert J.longest() <= 4300
    orc = E._Orc()
    want = J.want(orc, 0.15, MIN_ALN)
    orc.close()
    vol, ja = J.volume(hip, ctx)
    got = E._run(hip, ctx, monkeypatch, vol, ja, 0.15, MIN_ALN)
    cnt = _counters(ctx)
    narrow = E._run(hip, ctx, monkeypatch, vol, ja, 0.15, MIN_ALN, MECAT_CNS_WAVES="4")
    one = E._run(hip, ctx, monkeypatch, vol, ja, 0.15, MIN_ALN, MECAT_CNS_KERNEL="1")
    vol.free()
    print("cns_forward: %d jobs, the oracle accepts %.0f %%, rows relocated %d, tail-walk steps through a link %d, units handed over %d"
          % ((len(J), 100 * E._share_ok2(want)) + cnt))
    E._check_all(hip, J, got[0], got[1], want, "ring")
    assert E._same(got, narrow), "the default grid and four waves differ"
    assert E._same(got, one), "the default path and cns_extend differ"
    assert one[2] == 0                                            # (cns_forward did not run)
    assert cnt[0] > 0 and cnt[1] > 0
