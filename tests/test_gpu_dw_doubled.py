"""dw_extend2's d-row loops against the oracle's DiffAligner restatement and against the one-unit kernel (dw_extend), at the smallest
shapes at which a change of the row code's arithmetic — how positions, ring offsets and band limits are formed — can go wrong:

* identical sequences: snakes of 16 bases and more run across word ends and into the end of the block;
* last blocks of 1, 15, 16, 17, 511 - 513, 599 and 600 bases on the shorter side, alone and behind a full block, with the other sequence
  1.0 x and 1.2 x as long (718 bases: the longest block), both strands;
* error rates 0, 0.05, 0.15 and 0.30 per read;
* one insertion of 40 or of 70 bases in one of the two sequences: the band of that half passes 32 and 64 diagonals (rows of two and of
  three passes) and the band update cuts more than 31 diagonals at once;
* an unrelated pair (no end is reached: hand-over) and a job at qstart = sstart = 0 (an empty left extension).

Every job is compared field by field, once with so few waves that every half-wave runs many units and blocks one after the other."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

MIN_ALN = 500
FIELDS = ("ok", "query_start", "query_end", "target_start", "target_end", "matches", "columns")
EDGES = (1, 15, 16, 17, 511, 512, 513, 599, 600)
ERRORS = (0.0, 0.05, 0.15, 0.30)


@pytest.fixture(scope="module")
def hip():
    import mecat_amd.hip as M
    return M


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


def _mutate(rng, s, e):
    """substitutions, deletions and insertions at a total rate of about e (the mix of test_gpu_align._mutate), vectorised"""
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
    g = rng.integers(0, 4, size=3 * n + 64).astype(np.int8)
    q, t = _mutate(rng, g, e), _mutate(rng, g, e)
    assert len(q) >= nq and len(t) >= nt
    return q[:nq], t[:nt]


def _pair(rng, left, right, e):
    """(q, t, qstart, tstart): left / right = (query bases, target bases) on that side of the seed point"""
    ql, tl = _arm(rng, left[0], left[1], e)
    qr, tr = _arm(rng, right[0], right[1], e)
    return np.concatenate([ql[::-1], qr]), np.concatenate([tl[::-1], tr]), len(ql), len(tl)


class _Jobs:
    """a job list over a volume of its own, with the oracle's answer per job"""

    def __init__(self):
        self.seqs, self.jobs, self.want = [], [], []
        self.al = H.orc().orc_aligner_new()

    def add(self, q, t, qs, ts, chain):
        stored_q = (3 - q[::-1]).astype(np.int8) if chain else q          # the volume holds the read as sequenced
        i = len(self.seqs)
        self.seqs += [stored_q, t]
        self.jobs.append((i, i + 1, chain, qs, ts))
        q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
        o = H.OrcAlnResult()
        H.orc().orc_dw_go(self.al, q.ctypes.data, qs, len(q), t.ctypes.data, ts, len(t), MIN_ALN, C.byref(o))
        self.want.append((o.ok, o.query_start, o.query_end, o.target_start, o.target_end, o.matches, o.columns))

    def volume(self, hip, ctx):
        seqs = self.seqs + [np.zeros(64, np.int8)]                        # (no job's read is the last of the volume)
        lens = np.array([len(s) for s in seqs], dtype=np.int32)
        ov = H.orc_pack(np.concatenate(seqs).astype(np.uint8), lens)
        offs, pac = H.vol_arrays(ov)
        return hip.Volume(ctx, pac, offs, ov.contents.num_bases, 0)

    def close(self):
        H.orc().orc_aligner_free(self.al)


def _build_jobs():
    rng = np.random.default_rng(90210)
    J = _Jobs()
    # last-block sizes, alone and behind a full block (496: what a full block of identical sequences advances by)
    for e in ERRORS:
        for n in EDGES:
            for ratio in (1.0, 1.2):
                for pre in (0, 496):
                    chain = (n + pre // 496 + int(ratio > 1)) & 1
                    short, long_ = pre + n, pre + int(round(n * ratio))
                    q, t, qs, ts = _pair(rng, (short, long_), (long_, short), e)
                    J.add(q, t, qs, ts, chain)
                    J.add(t, q, ts, qs, 1 - chain)
    # one insertion of 40 / 70 bases in the query or in the target, 60 - 400 bases behind the seed point on either side
    for it in range(96):
        e = (0.0, 0.05, 0.15)[it % 3]
        ins = (40, 70)[(it // 3) & 1]
        L = int(rng.integers(1400, 2800))
        g = rng.integers(0, 4, size=L).astype(np.int8)
        s = int(rng.integers(500, L - 500))
        at = s + int(rng.integers(60, 400)) * (1 if it & 8 else -1)
        parts = [g[:min(s, at)], g[min(s, at):max(s, at)], g[max(s, at):]]
        qp, tp = [_mutate(rng, p, e) for p in parts], [_mutate(rng, p, e) for p in parts]
        extra = rng.integers(0, 4, size=ins).astype(np.int8)
        side = qp if it & 16 else tp
        k = 0 if at < s else 2                     # the insertion sits at `at`: the far end of the piece next to the seed point
        side[k] = np.concatenate([side[k], extra]) if at < s else np.concatenate([extra, side[k]])
        ks = 2 if at < s else 1                    # pieces in front of the seed point
        q, t = np.concatenate(qp), np.concatenate(tp)
        qs, ts = sum(len(p) for p in qp[:ks]), sum(len(p) for p in tp[:ks])
        for chain in (0, 1):
            J.add(q, t, qs, ts, chain)
    # reads of 1 - 3 kb with seed points at corresponding places: full blocks and last blocks of every size
    for it in range(700):
        e = ERRORS[it % 4]
        cuts = np.sort(rng.integers(0, int(rng.integers(1000, 2400)), size=3))
        L = int(rng.integers(int(cuts[2]) + 1, int(cuts[2]) + 700))
        g = rng.integers(0, 4, size=L).astype(np.int8)
        qp = [_mutate(rng, p, e) for p in np.split(g, cuts)]
        tp = [_mutate(rng, p, e) for p in np.split(g, cuts)]
        if it % 10 == 0:
            tp[3] = tp[3][: len(tp[3]) // 2]             # unequal rests: qblk != tblk in the last block
        if it % 10 == 5:
            qp[0] = qp[0][len(qp[0]) // 3:]
        q, t = np.concatenate(qp), np.concatenate(tp)
        if len(q) < 20 or len(t) < 20:
            continue
        for k in (1, 2, 3):
            qs, ts = sum(len(p) for p in qp[:k]), sum(len(p) for p in tp[:k])
            J.add(q, t, min(qs, len(q) - 1), min(ts, len(t) - 1), (it + k) & 1)
    # an unrelated pair; identical reads extended from their first base
    J.add(rng.integers(0, 4, size=2500).astype(np.int8), rng.integers(0, 4, size=2600).astype(np.int8), 1200, 1300, 0)
    g = rng.integers(0, 4, size=1800).astype(np.int8)
    J.add(g, g.copy(), 0, 0, 0)
    return J


def _run(hip, ctx, gv, jobs):
    out = hip.align_candidates(ctx, gv, gv, np.array(jobs, dtype=hip.JOB_DTYPE), MIN_ALN)
    return [tuple(int(r[f]) for f in FIELDS) for r in out]


def _diff(got, J):
    return [(i, J.jobs[i], got[i], J.want[i]) for i in range(len(got)) if got[i] != J.want[i]]


def test_row_loops_match_oracle_and_one_unit_kernel(hip, ctx, monkeypatch):
    J = _build_jobs()
    n = len(J.jobs)
    accepted = sum(w[0] for w in J.want)
    print("%d jobs, the oracle accepts %d" % (n, accepted))
    assert n > 2500 and accepted > 1000
    assert max(len(s) for s in J.seqs) <= 3750                  # (stretches of at most 3.1 kb; the mutations add a few percent)
    gv = J.volume(hip, ctx)
    monkeypatch.delenv("MECAT_DW_KERNEL", raising=False)
    monkeypatch.delenv("MECAT_DW_WAVES", raising=False)
    wide = _run(hip, ctx, gv, J.jobs)
    monkeypatch.setenv("MECAT_DW_WAVES", "4")
    narrow = _run(hip, ctx, gv, J.jobs)
    monkeypatch.delenv("MECAT_DW_WAVES")
    monkeypatch.setenv("MECAT_DW_KERNEL", "1")
    single = _run(hip, ctx, gv, J.jobs)
    bad = _diff(wide, J)
    assert not bad, "dw_extend2: %d/%d differ from the oracle: %s" % (len(bad), n, bad[:4])
    bad = _diff(narrow, J)
    assert not bad, "dw_extend2 on four waves: %d/%d differ from the oracle: %s" % (len(bad), n, bad[:4])
    bad = [(i, J.jobs[i], wide[i], single[i]) for i in range(n) if wide[i] != single[i]]
    assert not bad, "dw_extend2 and dw_extend differ on %d/%d: %s" % (len(bad), n, bad[:4])
    J.close()
    gv.free()
