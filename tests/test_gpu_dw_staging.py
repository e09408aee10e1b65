"""dw_extend2's word-interleaved staging and its single select per pass against the oracle's DiffAligner restatement and the one-unit
kernel (dw_extend), and the same pairs through cns_forward (dw_extend2<true>) against what test_gpu_cns_forward_edges compares with.

The staged words of a workgroup's eight half-waves share one array, word w of half u at dword 8 w + u, and a window's address is formed
from the doubled position by an AND; idle lanes' x + y is formed from the separator register (about -2^29), not selected.  The shapes are
the smallest at which either can go wrong:

* distinct neighbours: 17 pairs, every one from a random stretch of its own, so a word read from the neighbouring half's column (dword
  8 w + u +- 1) cannot match by accident; the list is also run alone on one workgroup, where all eight halves are live, run unlike units
  side by side and do not run out of units together;
* second staging trip: last blocks of 513, 528, 529, 600, 717 and 718 bases on the longer side (words 32 .. 44), as the only block and
  behind a full block, with a substitution 1 or 17 bases in front of the end of the shorter side, so the last words are compared (up to
  600 bases the longer side has one extra base near the block's start: both sequences are walked to their ends);
* word seams: identical arms with 1 .. 3 extra target bases near the seed point and a substitution at x = 16 k + 15, 16, 17: the main
  diagonal's snake ends and starts at a word seam of the query while the target's window straddles another;
* stale words: four pairs whose arms are 700-base last blocks at the head of a list of pairs with arms of 20 - 100 bases, alone on one
  workgroup: every half takes a long block first and short ones behind it, which see its words 2 .. 44;
* idle lanes against a small maximum: identical, homopolymer and (AC)n arms of 40 - 200 bases (one to three diagonals alive, x + y near
  0 in the first rows), and 15 %-error pairs of 1 - 3 kb (rows of exactly 32 slots, two-pass rows);
* four unrelated pairs: the hand-over path, seen in debug counter 8.

Every job is compared field by field with the oracle at the default grid and on four waves (one workgroup), and with dw_extend.  The
oracle accepts every pair that is meant to align."""
import numpy as np
import pytest

import test_gpu_cns_forward_edges as E
from test_gpu_dw_doubled import MIN_ALN, _mutate
from test_gpu_dw_snake_end import _DwJobs, _join, _run, _same_arm

pytestmark = pytest.mark.gpu

SECOND_TRIP = ((513, 512), (528, 527), (529, 528), (600, 599), (717, 598), (718, 599))      # (longer side, shorter side) of a last block
FULL = 496                     # what a full block of identical sequences advances by
ANCHOR = 560                   # an identical arm that makes a pair long enough to be accepted


@pytest.fixture(scope="module")
def hip():
    import mecat_amd.hip as M
    return M


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


def _sub(a, at, by=1):
    a[at] = (a[at] + by) & 3


def _pair_15(rng, lo, hi):
    """a 15 %-error pair of lo .. hi bases from a stretch of its own, seed point inside"""
    L = int(rng.integers(lo, hi))
    g = rng.integers(0, 4, size=L).astype(np.int8)
    cut = int(rng.integers(300, L - 300))
    qp, tp = [_mutate(rng, p, 0.15) for p in np.split(g, [cut])], [_mutate(rng, p, 0.15) for p in np.split(g, [cut])]
    return np.concatenate(qp), np.concatenate(tp), len(qp[0]), len(tp[0])


def _distinct(rng):
    return [_pair_15(rng, 900, 1500) + (it & 1, True) for it in range(17)]


def _second_trip(rng):
    out = []
    for long_, short in SECOND_TRIP:
        for pre in (0, FULL):
            for back in (1, 17):
                g = rng.integers(0, 4, size=pre + long_ + 8).astype(np.int8)
                s = g[: pre + short].copy()
                _sub(s, pre + short - back, 1 + (back & 1))
                if long_ <= 600:        # one extra base behind the block's seventh: both sequences end together
                    l = np.concatenate([g[: pre + 7], [(g[pre + 7] + 1) & 3], g[pre + 7: pre + long_ - 1]]).astype(np.int8)
                else:
                    l = g[: pre + long_].copy()
                assert len(s) == pre + short and len(l) == pre + long_
                chain = (long_ + back + pre) & 1
                q, t, qs, ts = _join((s, l), _same_arm(rng, 100, 100)) if back == 1 else _join(_same_arm(rng, 100, 100), (s, l))
                out.append((q, t, qs, ts, chain, True))
                out.append((t, q, ts, qs, 1 - chain, True))
    return out


def _seams(rng):
    out = []
    for extra in (1, 2, 3):
        for e in (15, 16, 17):
            g = rng.integers(0, 4, size=260).astype(np.int8)
            q = g.copy()
            for k in (2, 5, 9, 12):                       # the snake on the main diagonal ends at 16 k + e and starts behind it
                _sub(q, 16 * k + e, 1 + (k + e) % 3)
            t = np.concatenate([g[:5], rng.integers(0, 4, size=extra), g[5:]]).astype(np.int8)
            arm, anchor = (q, t), _same_arm(rng, ANCHOR, ANCHOR)
            q2, t2, qs, ts = _join(arm, anchor) if e & 1 else _join(anchor, arm)
            out.append((q2, t2, qs, ts, (extra + e) & 1, True))
            out.append((t2, q2, ts, qs, (extra + e + 1) & 1, True))
    return out


def _stale(rng):
    """four pairs with a 700-base last block on either side of the seed point, then pairs with one arm of 20 - 100 bases"""
    out = []
    for it in range(4):
        arms = []
        for side in range(2):
            g = rng.integers(0, 4, size=3 * 720).astype(np.int8)
            a, b = _mutate(rng, g, 0.10)[:599], _mutate(rng, g, 0.10)[:700 + it + side]
            arms.append((a, b) if (it + side) & 1 else (b, a))
        out.append(_join(arms[0], arms[1]) + (it & 1, True))
    for it in range(24):
        n = 20 + (it * 37) % 81
        g = rng.integers(0, 4, size=3 * n + 64).astype(np.int8)
        arm = (_mutate(rng, g, 0.15)[:n], _mutate(rng, g, 0.15)[: n + it % 5])
        anchor = _same_arm(rng, ANCHOR, ANCHOR)
        out.append((_join(arm, anchor) if it & 1 else _join(anchor, arm)) + ((it >> 1) & 1, True))
    return out


def _idle(rng):
    out = []
    units = (None, np.array([0], np.int8), np.array([0, 1], np.int8))        # a random stretch, A homopolymer, (AC)n
    for it, n in enumerate((40, 41, 63, 64, 65, 97, 128, 160, 200)):
        for unit in units:
            g = rng.integers(0, 4, size=n + 3).astype(np.int8) if unit is None else np.tile(unit, n)[: n + 3]
            arm = (g[:n].copy(), g[: n + it % 4].copy())
            anchor = _same_arm(rng, ANCHOR, ANCHOR)
            q, t, qs, ts = _join(arm, anchor) if it & 1 else _join(anchor, arm)
            out.append((q, t, qs, ts, it & 1, True))
            out.append((t, q, ts, qs, 1 - (it & 1), True))
    out += [_pair_15(rng, 1000, 3000) + (it & 1, True) for it in range(12)]
    return out


def _unrelated(rng):
    return [(rng.integers(0, 4, size=2500).astype(np.int8), rng.integers(0, 4, size=2600).astype(np.int8), 1200, 1300, it & 1, False)
            for it in range(4)]


@pytest.fixture(scope="module")
def groups():
    rng = np.random.default_rng(81216)
    g = {"distinct": _distinct(rng), "second trip": _second_trip(rng), "seams": _seams(rng), "stale": _stale(rng), "idle": _idle(rng),
         "unrelated": _unrelated(rng)}
    assert sum(len(v) for v in g.values()) & 1, "an odd number of jobs: a half ends without a unit while its partner rows on"
    return g


def _against_oracle(what, J, got):
    n = len(J.jobs)
    bad = [(i, J.jobs[i], got[i], J.want[i]) for i in range(n) if got[i] != J.want[i]]
    assert not bad, "%s: %d/%d differ from the oracle: %s" % (what, len(bad), n, bad[:4])


def test_staging_matches_oracle_and_one_unit_kernel(hip, ctx, groups, monkeypatch):
    cases = [c for v in groups.values() for c in v]
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
    _against_oracle("dw_extend2", J, wide)
    _against_oracle("dw_extend2 on four waves", J, narrow)
    bad = [(i, J.jobs[i], wide[i], single[i]) for i in range(n) if wide[i] != single[i]]
    assert not bad, "dw_extend2 and dw_extend differ on %d/%d: %s" % (len(bad), n, bad[:4])


@pytest.mark.parametrize("group", ["distinct", "stale"])
def test_one_workgroup_alone(hip, ctx, groups, monkeypatch, group):
    """the list alone on four waves: its units meet in the eight halves of one workgroup, in the list's order"""
    J = _DwJobs(groups[group])
    assert all(w[0] for w in J.want), "the oracle rejects a pair of the %s list" % group
    gv = J.volume(hip, ctx)
    monkeypatch.delenv("MECAT_DW_KERNEL", raising=False)
    monkeypatch.setenv("MECAT_DW_WAVES", "4")
    got, _ = _run(hip, ctx, gv, J.jobs)
    monkeypatch.delenv("MECAT_DW_WAVES")
    gv.free()
    _against_oracle("%s alone on four waves" % group, J, got)


def test_staging_in_cns_forward(hip, ctx, groups, monkeypatch):
    """the same pairs under mecat2cns' block rules: oracle (orc_cns_dw, orc_cns_get_alignment, both aligned strings), cns_extend, four waves"""
    J = E._Jobs()
    for v in groups.values():
        for q, t, qs, ts, chain, _ in v:
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
    E._check_all(hip, J, got[0], got[1], want, "staging")
    assert E._same(got, narrow), "the default grid and four waves differ"
    assert E._same(got, one), "the default path and cns_extend differ"
    assert one[2] == 0                                            # (cns_forward did not run)
