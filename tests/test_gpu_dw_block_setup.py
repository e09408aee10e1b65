"""dw_extend2's block set-up: the staging writes only the words that hold bases of the block, so the words behind it keep what an
earlier block (or an earlier unit of the same half-wave) left there.  No result may depend on them: last blocks at the sizes where the
staged word count, the second staging trip (blocks of more than 512 bases) and the block rules change, against the oracle's DiffAligner
restatement; and a job list run in two orders, so that every block meets two different histories of its half-wave's staging area."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

MIN_ALN = 500
FIELDS = ("ok", "query_start", "query_end", "target_start", "target_end", "matches", "columns")
# last-block sizes on the shorter side: around one base, one word, the full block (500), the 32-word trip (512), word edges
# behind it, and the block rule's limit (a rest below 600 is one block)
EDGES = (1, 15, 16, 17, 496, 499, 500, 501, 511, 512, 513, 527, 528, 529, 599, 600)


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
    g = rng.integers(0, 4, size=2 * n + 64).astype(np.int8)
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


def _run(hip, ctx, gv, jobs):
    out = hip.align_candidates(ctx, gv, gv, np.array(jobs, dtype=hip.JOB_DTYPE), MIN_ALN)
    return [tuple(int(r[f]) for f in FIELDS) for r in out]


def test_last_block_size_edges(hip, ctx):
    """Every edge size as the last block of the left and of the right extension, alone and behind one full block, with the other
    sequence 1.0 x and 1.2 x as long (the longer block then reaches 718 bases), both strands, at error rates 0 (identical sequences: the
    snake runs into the block end and looks into the words behind it), 0.05 and 0.15; and one unrelated pair that stops early."""
    rng = np.random.default_rng(20240)
    J = _Jobs()
    for e in (0.0, 0.05, 0.15):
        for n in EDGES:
            for ratio in (1.0, 1.2):
                for pre in (0, 496):                     # 496: what a full block of identical sequences advances by
                    chain = (n + pre // 496 + int(ratio > 1)) & 1
                    short, long_ = pre + n, pre + int(round(n * ratio))
                    # the query is the shorter side on the left of the seed point, the target on the right
                    q, t, qs, ts = _pair(rng, (short, long_), (long_, short), e)
                    J.add(q, t, qs, ts, chain)
                    J.add(t, q, ts, qs, 1 - chain)
    J.add(rng.integers(0, 4, size=2500).astype(np.int8), rng.integers(0, 4, size=2600).astype(np.int8), 1200, 1300, 0)
    gv = J.volume(hip, ctx)
    got = _run(hip, ctx, gv, J.jobs)
    bad = [(i, J.jobs[i], got[i], J.want[i]) for i in range(len(got)) if got[i] != J.want[i]]
    assert not bad, "%d/%d differ: %s" % (len(bad), len(got), bad[:4])
    assert sum(w[0] for w in J.want) > 100
    J.close()
    gv.free()


def test_results_do_not_depend_on_staging_history(hip, ctx, monkeypatch):
    """About 3 000 jobs on reads of 1 - 3 kb (full blocks, and last blocks from a few bases to 700), with so few waves that every
    half-wave runs several units one after the other: in the given order and in a permuted one each job must give the oracle's answer,
    and the one-unit kernel (dw_extend, which stages every block afresh in its own layout) as well."""
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
            tp[3] = tp[3][: len(tp[3]) // 2]             # unequal rests: qblk != tblk in the last block
        if it % 10 == 5:
            qp[0] = qp[0][len(qp[0]) // 3:]
        q, t = np.concatenate(qp), np.concatenate(tp)
        if len(q) < 20 or len(t) < 20:
            continue
        for k in (1, 2, 3):                                  # seed points at the piece boundaries: they correspond exactly
            qs, ts = sum(len(p) for p in qp[:k]), sum(len(p) for p in tp[:k])
            J.add(q, t, min(qs, len(q) - 1), min(ts, len(t) - 1), (it + k) & 1)
    gv = J.volume(hip, ctx)
    n = len(J.jobs)
    perm = rng.permutation(n)
    monkeypatch.setenv("MECAT_DW_WAVES", "4")
    first = _run(hip, ctx, gv, J.jobs)
    second = _run(hip, ctx, gv, [J.jobs[i] for i in perm])
    monkeypatch.setenv("MECAT_DW_KERNEL", "1")
    single = _run(hip, ctx, gv, J.jobs)
    bad = [(i, J.jobs[i], first[i], J.want[i]) for i in range(n) if first[i] != J.want[i]]
    assert not bad, "given order: %d/%d differ from the oracle: %s" % (len(bad), n, bad[:4])
    bad = [(int(i), J.jobs[i], second[k], J.want[i]) for k, i in enumerate(perm) if second[k] != J.want[i]]
    assert not bad, "permuted order: %d/%d differ from the oracle: %s" % (len(bad), n, bad[:4])
    bad = [(i, J.jobs[i], single[i], J.want[i]) for i in range(n) if single[i] != J.want[i]]
    assert not bad, "dw_extend: %d/%d differ from the oracle: %s" % (len(bad), n, bad[:4])
    assert [second[k] for k in np.argsort(perm)] == first
    assert n > 2900 and sum(w[0] for w in J.want) > 1000
    J.close()
    gv.free()
