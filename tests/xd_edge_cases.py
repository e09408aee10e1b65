"""Deterministic inputs that put the X-drop block (mecat_amd/csrc/xd_block_ring.h, xd_block_wide.h, XTail in xd_defs.h) at its window,
traceback and trim edges, and a walker that says, from the oracle alone, what every block of every job does there.

The walker is align_ex and XdropAligner::go (common/xdrop_gapalign.cpp:263-439) restated in Python over oracle/liboracle.so's
orc_xdrop_align_trace: Python does the chaining of the blocks, script_to_aligned_string and trim_mismatch_end (a few lines each); the
block itself, with the window of every row, is the oracle's.  tests/test_xd_edge_cases_cpu.py pins the oracle to the compiled reference on
exactly these inputs, checks that the walker's results equal orc_xdrop_go's, and asserts the premises each family was built for.

Sequences are codes 0..3 (a, c, g, t).  A family is a Cases object: .seqs (the reads as a volume stores them: the query reversed and
complemented where the job's chain is 1), .jobs (qid, sid, chain, qstart, sstart: tests/test_gpu_xalign.py's form) and .pairs (the query on
the job's strand, the target, the start point, a label)."""
import ctypes as C

import numpy as np

import helpers as H

GAP = 4
X_SUB, X_GAP_IN_A, X_GAP_IN_B = 3, 0, 6          # xdrop_gapalign.h:13-34: a column with both bases, a target base only, a query base only
SEG = 500
RING_CELLS = 126                                 # the ring block holds a window of XW_RING - 2 cells
FIELDS = ("ok", "query_start", "query_end", "target_start", "target_end", "matches", "columns")
A_, C_, G_, T_ = 0, 1, 2, 3

_xa = None


def xaligner():
    global _xa
    if _xa is None:
        _xa = H.orc().orc_xaligner_new()
    return _xa


# ----------------------------------------------------------------------------- the walker
def block(q, t, forward=1):
    """one xdrop_align of the block (q, t), both in EXTENSION order -> dict: ae, be, score-free facts of the rows (rows entered, cells =
    the sum of the windows at the rows' entries, widest = the widest window a row left behind, measured as the ring block measures it),
    qstr / tstr (script_to_aligned_string, extension order, GAP = 4), and of the traceback path: idx[i] = the index inside its row's
    window of the cell the walk stood on before its i-th step (-1 for a cell of row 0), gap[i] = that step was not a substitution; q, t,
    forward, ops = the call's own arguments (the arrays as the oracle reads them) and its edit block"""
    M, N = len(q), len(t)
    out = dict(M=M, N=N, ae=0, be=0, rows=0, cells=0, widest=0, qstr=np.zeros(0, np.int8), tstr=np.zeros(0, np.int8),
               idx=np.zeros(0, np.int64), gap=np.zeros(0, bool))
    if M <= 0 or N <= 0:
        return out
    qa = np.ascontiguousarray(q if forward else q[::-1], dtype=np.int8)
    ta = np.ascontiguousarray(t if forward else t[::-1], dtype=np.int8)
    res = np.zeros(3, np.int32)
    ops = np.zeros(2 * (M + N + 2), np.int32)
    fb, bs = np.zeros(M + 1, np.int32), np.zeros(M + 1, np.int32)
    rows = H.orc().orc_xdrop_align_trace(xaligner(), qa.ctypes.data, M, ta.ctypes.data, N, int(forward), res.ctypes.data, ops.ctypes.data,
                                         fb.ctypes.data, bs.ctypes.data)
    ae, be, nops = (int(x) for x in res)
    fb, bs = fb[: rows + 1].astype(np.int64), bs[: rows + 1].astype(np.int64)
    out.update(ae=ae, be=be, rows=rows, cells=int((bs[:rows] - fb[:rows]).sum()), fb=fb, bs=bs, q=qa, t=ta, forward=int(forward), ops=ops[: 2 * nops].copy())
    # what row a leaves behind: the next row's window, and its end counted from this row's own first column
    out["widest"] = int(np.maximum(bs[1:] - fb[1:], bs[1:] - fb[:-1]).max()) if rows else 0
    op = np.repeat(ops[0: 2 * nops: 2], ops[1: 2 * nops: 2])          # the steps from (ae, be) towards (0, 0)
    da, db = (op != X_GAP_IN_A).astype(np.int64), (op != X_GAP_IN_B).astype(np.int64)
    a = ae - np.concatenate([[0], np.cumsum(da)[:-1]])                # the cell in front of every step
    b = be - np.concatenate([[0], np.cumsum(db)[:-1]])
    assert int(da.sum()) == ae and int(db.sum()) == be
    out["idx"] = np.where(a >= 1, b - fb[np.maximum(a, 1) - 1], -1)
    out["gap"] = op != X_SUB
    assert (out["idx"][a >= 1] >= 0).all() and (b[a >= 1] < bs[np.minimum(a, rows)][a >= 1]).all(), "a path cell outside its row's window"
    # script_to_aligned_string: the steps in reverse are the columns in extension order
    fo = op[::-1]
    qi, ti = np.cumsum(fo != X_GAP_IN_A) - 1, np.cumsum(fo != X_GAP_IN_B) - 1
    qe, te = np.asarray(q, dtype=np.int8), np.asarray(t, dtype=np.int8)
    out["qstr"] = np.where(fo != X_GAP_IN_A, qe[np.maximum(qi, 0)], GAP).astype(np.int8)
    out["tstr"] = np.where(fo != X_GAP_IN_B, te[np.maximum(ti, 0)], GAP).astype(np.int8)
    return out


def trim_mismatch_end(qstr, tstr, mat=4):
    """gapalign.cpp:47-68 -> (ok, qcnt, tcnt, acnt, a run of `mat` matches was found): from the last column backwards through the first
    run of `mat` equal columns; ok if there is one and at least two columns lie in front of it"""
    n = len(qstr)
    eq = (qstr == tstr)[::-1]
    run = eq[: max(n - mat + 1, 0)].copy()
    for i in range(1, mat):
        run &= eq[i: n - mat + 1 + i]
    found = bool(run.any())
    acnt = int(np.argmax(run)) + mat if found else n
    qcnt, tcnt = int((qstr[n - acnt:] != GAP).sum()), int((tstr[n - acnt:] != GAP).sum())
    return found and n - acnt - 1 > 0, qcnt, tcnt, acnt, found


def column_kind(qc, tc):
    """M: equal bases, S: a substitution, Q: a query base only, T: a target base only"""
    return "T" if qc == GAP else "Q" if tc == GAP else "M" if qc == tc else "S"


def direction(q, t, forward):
    """align_ex over the direction's two sequences in extension order -> (blocks, qstr, tstr): every block as block() gives it plus
    qleft, tleft (what is left of the two sides in front of it), qblk, tblk, last, full_map, used (its columns went into the strings), and for a full-mapped block that is not the last: trim_ok,
    found (a run of four matches exists), acnt, kept (= n - acnt) and l1 (the kind of the column in front of the trimmed tail)"""
    qsize, tsize = max(len(q), 0), max(len(t), 0)
    qidx = tidx = 0
    blocks, qs, ts = [], [], []
    while True:
        qleft, tleft = qsize - qidx, tsize - tidx
        if qleft < SEG + 100 or tleft < SEG + 100:
            qblk, tblk, last = min(qleft, int(tleft + tleft * 0.2)), min(tleft, int(qleft + qleft * 0.2)), True
        else:
            qblk, tblk, last = SEG, SEG, False
        b = block(q[qidx: qidx + qblk], t[tidx: tidx + tblk], forward)
        n = len(b["qstr"])
        b.update(qleft=qleft, tleft=tleft, qblk=qblk, tblk=tblk, last=last, n=n, full_map=(qblk - b["ae"] <= 20 or tblk - b["be"] <= 20), used=False, trim_ok=None)
        blocks.append(b)
        if not b["full_map"] or last:
            qs.append(b["qstr"]); ts.append(b["tstr"])
            b["used"] = True
            break
        ok, qcnt, tcnt, acnt, found = trim_mismatch_end(b["qstr"], b["tstr"])
        b.update(trim_ok=bool(ok), found=bool(found), acnt=acnt, kept=n - acnt,
                 l1=column_kind(b["qstr"][n - acnt - 1], b["tstr"][n - acnt - 1]) if n - acnt >= 1 else None)
        if not ok:
            break
        qs.append(b["qstr"][: n - acnt]); ts.append(b["tstr"][: n - acnt])
        b["used"] = True
        qidx += b["ae"] - qcnt
        tidx += b["be"] - tcnt
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int8)
    return blocks, cat(qs), cat(ts)


def walk(q, qs, t, ts):
    """XdropAligner::go for the query q (on the job's strand) from the start point (qs, ts) -> dict(res = the seven result fields without
    ok's threshold applied: (span, query_start, ...), left / right = the blocks, lq / lt / rq / rt = the strings of the two halves in
    extension order, the left one with its last column still on).  A start point in front of a read is a job without extension (the
    reference would read in front of its arrays there): one block of no rows per direction, nothing aligned."""
    q, t = np.asarray(q, dtype=np.int8), np.asarray(t, dtype=np.int8)
    if qs < 0 or ts < 0:
        e = np.zeros(0, np.int8)
        lb, lq, lt = direction(e, e, 0)
        rb, rq, rt = direction(e, e, 1)
    else:
        lb, lq, lt = direction(q[:qs][::-1], t[:ts][::-1], 0)
        rb, rq, rt = direction(q[qs:], t[ts:], 1)
    kq, kt = lq[: max(len(lq) - 1, 0)], lt[: max(len(lt) - 1, 0)]          # go leaves the left half's last column out (:401-402)
    r = dict(query_start=qs - int((kq != GAP).sum()), query_end=qs + int((rq != GAP).sum()),
             target_start=ts - int((kt != GAP).sum()), target_end=ts + int((rt != GAP).sum()),
             matches=int((kq == kt).sum() + (rq == rt).sum()), columns=len(kq) + len(rq))
    return dict(res=r, left=lb, right=rb, lq=lq, lt=lt, rq=rq, rt=rt)


def result_tuple(w, min_aln):
    r = w["res"]
    return (int(r["query_end"] - r["query_start"] >= min_aln),) + tuple(r[k] for k in FIELDS[1:])


def go(q, qs, t, ts, min_aln):
    """orc_xdrop_go -> the seven fields.  A start point in front of a read is the one case whose expected value comes from neither the
    oracle nor the reference (both would read in front of their arrays): it is written down here as "not extended", which is what
    xalign.hip's `dead` branch does and what tests/test_gpu_parity.py asks of such a job, so for those few jobs the test only says that
    the kernel leaves them alone and does not fault."""
    if qs < 0 or ts < 0:
        return (0, qs, qs, ts, ts, 0, 0)
    qc, tc = np.ascontiguousarray(q, dtype=np.int8), np.ascontiguousarray(t, dtype=np.int8)
    o = H.OrcAlnResult()
    H.orc().orc_xdrop_go(xaligner(), qc.ctypes.data, int(qs), len(qc), tc.ctypes.data, int(ts), len(tc), int(min_aln), C.byref(o))
    return tuple(int(getattr(o, f)) for f in FIELDS)


def strings(w):
    """the job's two aligned strings as go emits them (left half reversed and without its last column, then the right half)"""
    kq, kt = w["lq"][: max(len(w["lq"]) - 1, 0)], w["lt"][: max(len(w["lt"]) - 1, 0)]
    dt = np.frombuffer(b"ACGT-", dtype=np.uint8)
    return dt[np.concatenate([kq[::-1], w["rq"]])].tobytes(), dt[np.concatenate([kt[::-1], w["rt"]])].tobytes()


class Cases:
    def __init__(self, name):
        self.name, self.seqs, self.jobs, self.pairs, self._walks = name, [], [], [], None

    def add(self, q, t, qs, ts, chain, label=None):
        q, t = np.asarray(q, dtype=np.int8), np.asarray(t, dtype=np.int8)
        i = len(self.seqs)
        self.seqs.append((3 - q[::-1]).astype(np.int8) if chain else q)
        self.seqs.append(t)
        self.jobs.append((i, i + 1, int(chain), int(qs), int(ts)))
        self.pairs.append((q, t, int(qs), int(ts), label))

    def both_strands(self, q, t, qs, ts, label=None):
        for chain in (0, 1):
            self.add(q, t, qs, ts, chain, label)

    def walks(self):
        if self._walks is None:
            self._walks = [walk(q, qs, t, ts) for q, t, qs, ts, _ in self.pairs]
        return self._walks

    def units(self):
        """-> [(job, direction (0 = left), blocks)]"""
        return [(j, d, w[("left", "right")[d]]) for j, w in enumerate(self.walks()) for d in (0, 1)]

    def blocks(self):
        return [b for _, _, bl in self.units() for b in bl]

    def totals(self):
        bl = self.blocks()
        return dict(jobs=len(self.jobs), blocks=len(bl), rows=sum(b["rows"] for b in bl), cells=sum(b["cells"] for b in bl),
                    redone=sum(b["widest"] > RING_CELLS for b in bl), wide_units=sum(any(b["widest"] > RING_CELLS for b in u) for _, _, u in self.units()))

    def subset(self, keep, name):
        """the jobs whose pair passes keep(q, t, qs, ts, label), as a family of its own (reads renumbered)"""
        s = Cases(name)
        for (q, t, qs, ts, lab), jb in zip(self.pairs, self.jobs):
            if keep(q, t, qs, ts, lab):
                s.add(q, t, qs, ts, jb[2], lab)
        return s


def rand(rng, n):
    return rng.integers(0, 4, int(n)).astype(np.int8)


def rep(unit, n):
    return np.tile(np.array(unit, dtype=np.int8), n)


def cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.int8) for p in parts])


# ----------------------------------------------------------------------------- the families
def ladder_pair(R, k, mirrored):
    """60 random bases, then a x 40, ca x k, g x 60 against the same 60 bases and a x 400: every a of the query's stretch pairs with any a
    of the target's, so the window grows by one cell per ca (47 + k cells at its widest).  mirrored: the two reads swapped"""
    q = cat(R, rep([A_], 40), rep([C_, A_], k), rep([G_], 60))
    t = cat(R, rep([A_], 400))
    return (t, q) if mirrored else (q, t)


LADDER_K = tuple(range(10, 26)) + tuple(range(70, 91))


def family_a():
    """A. the window ladder: one last block per job from the start point (0, 0)"""
    rng = np.random.default_rng(7101)
    R = rand(rng, 60)
    cs = Cases("A")
    for mirrored in (0, 1):
        for k in LADDER_K:
            q, t = ladder_pair(R, k, mirrored)
            cs.both_strands(q, t, 0, 0, (k, mirrored))
    return cs


def through_pair(R, S, k, d, form, swapped):
    """a stretch the alignment comes through: a x 40, ca x k against a homopolymer of 40 + k + d (form 0: every c a query-only column),
    40 + 2 k + d (form 1: every c a substitution) or 40 + k - d bases (form 2), between the same random R in front and S behind"""
    q = cat(R, rep([A_], 40), rep([C_, A_], k), S)
    t = cat(R, rep([A_], (40 + k + d, 40 + 2 * k + d, 40 + k - d)[form]), S)
    return (t, q) if swapped else (q, t)


B_PARAMS = [(k, d, form, sw) for k in range(55, 63) for d in (0, 5, 10, 15, 20) for form, sw in ((0, 1), (1, 0), (2, 1))]


def family_b():
    """B. the traceback in the second chunk: the best cell lies behind the wide stretch, the walk goes back through it"""
    rng = np.random.default_rng(7102)
    R, S = rand(rng, 60), rand(rng, 200)
    cs = Cases("B")
    for k, d, form, sw in B_PARAMS:
        q, t = through_pair(R, S, k, d, form, sw)
        assert len(q) < 600 and len(t) < 718
        cs.both_strands(q, t, 0, 0, (k, d, form, sw))
    return cs


def realize(rng, cols, pq, pt):
    """the columns as bases, in the order given, behind the bases pq (query) and pt (target) -> (query bases, target bases).  No base
    equals its neighbour on either side, so a shift by one base never turns substitutions into matches"""
    draws = iter(rng.integers(0, 12, 2 * len(cols) + 2).tolist())          # (12: a multiple of every number of bases left to choose from)

    def pick(*avoid):
        left = [b for b in range(4) if b not in avoid]
        return left[next(draws) % len(left)]
    qb, tb = [], []
    for c in cols:
        if c == "M":
            pt = pq = pick(pt, pq); qb.append(pq); tb.append(pt)
        elif c == "S":
            b = pick(pt, pq); pq = pick(b, pt, pq) if pt != pq else pick(b, pt); pt = b
            qb.append(pq); tb.append(pt)
        elif c == "Q":       # a base on one side only
            pq = pick(pt, pq); qb.append(pq)
        else:
            pt = pick(pt, pq); tb.append(pt)
    return np.array(qb, dtype=np.int8), np.array(tb, dtype=np.int8)


REST_BG = 700          # "bg": the background goes on for this many columns behind block 1


def from_tail(rng, cols, rest="equal"):
    """two reads whose first block of 500 x 500 ends with the columns `cols`, listed from the block's LAST column backwards (M: equal
    bases, S: a substitution, Q: a query base only, T: a target base only); in front of them the reads are equal -> (q, t).
    xdrop_align never takes a block's last target base (b_size stops at N), so the columns end at target base 499 or at query base
    500, whichever comes first; the other side gets the rest of its 500 bases from the sequence behind, and with one side used up
    the block's best cell is still the planned last column.
    What lies behind decides what the trimmed tail is worth.  rest "equal": 650 equal bases, so block 2 re-aligns the tail and goes on,
    and every split of the same columns between the two blocks gives the same result.  rest "bg": the background (a substitution
    every fourth base) goes on through block 2, which then has its only run of four matches at its very first columns: its trim is
    refused, the direction ends with what block 1 KEPT, and acnt, qcnt, tcnt, the tail's matches and the type of the column in front of
    the tail all show in the result."""
    nq = sum(c != "T" for c in cols)
    nt = sum(c != "Q" for c in cols)
    p = min(SEG - nq, SEG - 1 - nt)
    assert p >= 0
    head = rand(rng, p)
    h = int(rng.integers(0, 4))
    qt, tt = realize(rng, cols, h, h)          # the tails, backwards
    pq, pt = (int(qt[0]) if len(qt) else h), (int(tt[0]) if len(tt) else h)
    if rest == "bg":
        rq, rt = realize(rng, ["S" if i % 4 == 0 else "M" for i in range(REST_BG)], pq, pt)
        same = rand(rng, 50)
        rq, rt = cat(rq, same), cat(rt, same)
    else:
        rq = rt = rand(rng, 650)
    q = cat(head, qt[::-1], rq)
    t = cat(head, tt[::-1], rt)
    return q, t


def background(n=100):
    """three matches and one substitution, repeating, from the tail: no run of four matches"""
    return ["S" if i % 4 == 3 else "M" for i in range(n)]


TAIL_PATTERNS = {          # from the tail backwards
    "m4": "MMMM", "m5": "MMMMM", "m8": "MMMMMMMM",
    "t.m4": "TMMMM", "q.m4": "QMMMM", "tt.m4": "TTMMMM",          # four matches behind (on the far side of) a gap
    "m4.t": "MMMMT", "m4.q": "MMMMQ", "m4.tt": "MMMMTT",          # four matches in front of a gap: the gap is the column before the trimmed tail
    "m3.s.m4": "MMMSMMMM",
}


def tail_cols(pattern, s, row15=False):
    """the background with the pattern s columns from the tail.  row15: four target-only columns far behind the pattern, so that the
    target's 499 bases are used up in the query's row 495 and the block's end point lies there"""
    cols = background(100)
    P = list(TAIL_PATTERNS[pattern])
    if s > 0 and P[0] == "M":
        cols[s - 1] = "S"          # the pattern's run starts at column s
    cols[s: s + len(P)] = P
    if P[-1] == "M" and pattern not in ("m5", "m8", "m3.s.m4"):
        cols[s + len(P)] = "S"     # ... and is four matches long
    if row15:
        cols[90:90] = ["T"] * 4
    return cols


def trim_edge_cols(d):
    """the background through the whole block, four matches at its very first columns with d = 0..3 columns in front of them (n - acnt =
    d); d = None: no run of four matches at all"""
    n = SEG - 1          # (the block's last target base is never taken)
    cols = background(n)
    if d is not None:
        cols[n - d:] = ["S"] * d
        cols[n - d - 4: n - d] = ["M"] * 4
        cols[n - d - 5] = "S"
    return cols


def to_the_left(q, t, rng):
    """the same pair as a LEFT extension: the reads reversed, 50 equal bases behind them, the start point at the reversed reads' end"""
    tail = rand(rng, 50)
    return cat(q[::-1], tail), cat(t[::-1], tail), len(q), len(t)


C_LEFT_S = tuple(range(0, 71, 7))
C_ROW15_S = tuple(range(26, 42))


def family_c():
    """C. tail patterns, exhaustive over the position: block 1 is a full-mapped 500 x 500 block that is not the last.  Every pattern at
    every position to the right and to the left with the background behind block 1 (see from_tail: the trimmed tail then shows in
    the result), and with equal sequence behind at every seventh position; positions 26..41 also with the block's end point in row
    495: the ring's traceback takes 32 columns in one turn only in its first turn from a row that is 15
    modulo 16.  Every one of them on both strands."""
    rng = np.random.default_rng(7103)
    cs = Cases("C")
    for name in TAIL_PATTERNS:
        for s in range(0, 71):
            cols = tail_cols(name, s)
            q, t = from_tail(rng, cols, "bg")
            cs.both_strands(q, t, 0, 0, ("tail", name, s, "bg", 1))
            ql, tl, qs, ts = to_the_left(q, t, rng)
            cs.both_strands(ql, tl, qs, ts, ("tail", name, s, "bg", 0))
            if s in C_LEFT_S:
                q, t = from_tail(rng, cols, "equal")
                cs.both_strands(q, t, 0, 0, ("tail", name, s, "equal", 1))
                ql, tl, qs, ts = to_the_left(q, t, rng)
                cs.both_strands(ql, tl, qs, ts, ("tail", name, s, "equal", 0))
            if s in C_ROW15_S:
                q, t = from_tail(rng, tail_cols(name, s, row15=True), "bg")
                cs.both_strands(q, t, 0, 0, ("tail", name, s, "bg495", 1))
                ql, tl, qs, ts = to_the_left(q, t, rng)
                cs.both_strands(ql, tl, qs, ts, ("tail", name, s, "bg495", 0))
    for d in (0, 1, 2, 3, None):
        q, t = from_tail(rng, trim_edge_cols(d))
        cs.both_strands(q, t, 0, 0, ("trim", d, 1))
        ql, tl, qs, ts = to_the_left(q, t, rng)
        cs.both_strands(ql, tl, qs, ts, ("trim", d, 0))
    return cs


D_SIDES = (599, 600, 601, 718, 719)
D_TARGET_SIDES = (1, 2, 29, 30, 31)
D_QUERY_SIDES = (1, 2, 63, 64, 65, 127, 128, 129)


def mutated(rng, s, e):
    """a copy of s with substitutions, insertions and deletions, a third of e each"""
    out = []
    for b in s:
        u = rng.random()
        if u < e / 3:
            continue
        if u < 2 * e / 3:
            out.append(int(rng.integers(0, 4)))
        out.append(int(b) if u >= e else int((b + 1 + rng.integers(0, 3)) % 4))
    return np.array(out, dtype=np.int8)


def family_d():
    """D. block geometry in xd_extend_w's own view"""
    rng = np.random.default_rng(7104)
    cs = Cases("D")
    L = rand(rng, 300)          # what lies on the other side of the start point

    def sided(qr, tr, right, chain, label):
        if right:
            cs.add(cat(L, qr), cat(L, tr), len(L), len(L), chain, label)
        else:
            cs.add(cat(qr[::-1], L), cat(tr[::-1], L), len(qr), len(tr), chain, label)
    G = rand(rng, 1000)
    for err in (0.0, 0.08):
        for sq in D_SIDES:
            for st in D_SIDES:
                for right in (1, 0):
                    for chain in (0, 1):
                        qm = mutated(rng, G, err)
                        assert len(qm) >= 719
                        sided(qm[:sq], G[:st], right, chain, ("sides", sq, st, right))
    long_side = rand(rng, 800)
    for n in D_TARGET_SIDES:
        for right in (1, 0):
            for chain in (0, 1):
                sided(long_side, long_side[:n], right, chain, ("target", n, right))
    for n in D_QUERY_SIDES:
        for right in (1, 0):
            for chain in (0, 1):
                sided(long_side[:n], long_side, right, chain, ("query", n, right))
                sided(mutated(rng, long_side, 0.08)[:n], long_side, right, chain, ("query", n, right))
    # full-map edges: block 1 equal for its first 479 / 480 bases, nothing that matches behind (a x .. against c x ..)
    for nq, nt in ((480, 480), (479, 479), (480, 479), (479, 480), (481, 478), (478, 481)):
        Cm = rand(rng, max(nq, nt))
        Cm[-1] = G_          # (the last equal base is neither of the two homopolymers)
        qc = Cm if nq >= nt else np.delete(Cm, np.arange(200, 200 + nt - nq))
        tc = Cm if nt >= nq else np.delete(Cm, np.arange(200, 200 + nq - nt))
        q, t = cat(qc, rep([A_], 700)), cat(tc, rep([C_], 700))
        for chain in (0, 1):
            cs.add(q, t, 0, 0, chain, ("fullmap", nq, nt, 1))
            ql, tl, qs, ts = to_the_left(q, t, rng)
            cs.add(ql, tl, qs, ts, chain, ("fullmap", nq, nt, 0))
    # a start point in front of a read: a job without extension
    for chain in (0, 1):
        for qs, ts in ((-5, 100), (100, -5), (-1, -1), (-700, 0)):
            cs.add(long_side, long_side, qs, ts, chain, ("negative", qs, ts))
    return cs


def family_e():
    """E. hand-over resumption: the block that outgrows the ring is a unit's second or third, to the right and to the left; two such
    blocks in one unit; ring blocks behind it"""
    rng = np.random.default_rng(7105)
    cs = Cases("E")
    for k, d, form, sw in ((85, 0, 0, 0), (90, 0, 0, 1), (88, 5, 0, 1), (95, 10, 0, 0), (86, 5, 1, 0), (92, 0, 2, 1)):
        for front in (700, 1000, 1300):
            P, S, S2 = rand(rng, front), rand(rng, 700), rand(rng, 900)
            mid = rand(rng, 600)
            q, t = through_pair(P, S, k, d, form, sw)
            cs.both_strands(q, t, 0, 0, ("right", k, front))
            cs.both_strands(q, t, len(q) - 30, len(t) - 30, ("left", k, front))
            cs.both_strands(q, t, len(q) - 400, len(t) - 400, ("left", k, front))
            none = np.zeros(0, np.int8)
            sq, st = through_pair(none, none, k, d, form, sw)
            q3, t3 = cat(P, sq, mid, sq, S2), cat(P, st, mid, st, S2)          # two wide stretches 600 bases apart
            cs.both_strands(q3, t3, 0, 0, ("two", k, front))
            cs.both_strands(q3, t3, len(q3) - 200, len(t3) - 200, ("two-left", k, front))
    return cs


FAMILIES = dict(A=family_a, B=family_b, C=family_c, D=family_d, E=family_e)
_made = {}


def family(name):
    """the family, made once per process (its walks are kept with it)"""
    if name not in _made:
        _made[name] = FAMILIES[name]()
    return _made[name]


def ladder_below():
    """the part of family A below the ring's limit, by its parameters: the plain pairs up to k = 79 (126 cells), the mirrored ones of
    the lower range"""
    if "A-below" not in _made:
        _made["A-below"] = family("A").subset(lambda q, t, qs, ts, lab: lab[0] <= (25 if lab[1] else 79), "A-below")
    return _made["A-below"]


def everything():
    """all five families as one list of jobs (more jobs than a small launch has waves: the longest-first order then really sorts)"""
    if "all" not in _made:
        s = Cases("all")
        for name in FAMILIES:
            f = family(name)
            for (q, t, qs, ts, lab), jb in zip(f.pairs, f.jobs):
                s.add(q, t, qs, ts, jb[2], (name, lab))
            s._walks = (s._walks or []) + f.walks()
        _made["all"] = s
    return _made["all"]


# ----------------------------------------------------------------------------- the same pairs as mecat2ref sees them (ref_xextend)
REF_PARTS = 4          # "C/0" .. "C/3": a family in quarters, each with a reference of its own (every job is in one of them)
REF_PREFIX = 1100          # families A and B: equal bases in front of the start point, so that the query span passes extend_candidate's 1 000


def ref_view(name):
    """family A, B, C or E, every job of it (or its quarter "C/0" .. "C/3"), for mhip_ref_xextend_run: the targets as a multi-sequence reference, the queries as reads, one candidate per job
    -> dict(text = the reference FASTA, reads = [letters], cands int64[m, 5], labels = the pairs' labels, walks = walk() of every candidate on extract_sequences'
    window of the concatenated reference (tests/ref_ext_ref.py: window), codes = the concatenated reference).  The window is cut from the
    whole reference, so a target's block may reach into the sequence behind it: the walks are this view's own.  A and B get REF_PREFIX
    equal random bases in front of both reads and start behind them: the right half is still the family's single block; C gets 700
    equal bases on the other side of the start point.  Either way the query span passes 1 000 and the strings are there to compare."""
    import ref_cand_cases as RC
    import ref_ext_cases as XC
    import ref_ext_ref as X
    key = "ref-" + name
    if key not in _made:
        name, _, part = name.partition("/")
        f = family(name)
        rng = np.random.default_rng(7200 + ord(name))
        P = rand(rng, REF_PREFIX if name in "AB" else 0)
        names, seqs, reads, cands, starts = [], [], [], [], []
        at = 0
        more = rand(rng, 700 if name == "C" else 0)
        none = np.zeros(0, np.int8)
        lo, hi = (0, len(f.jobs)) if not part else (len(f.jobs) * int(part) // REF_PARTS, len(f.jobs) * (int(part) + 1) // REF_PARTS)
        for (q, t, qs, ts, lab), jb in zip(f.pairs[lo:hi], f.jobs[lo:hi]):
            # family C: 700 equal bases on the far side of the start point (many of its units end with block 1's 460 columns)
            front, back = (P, none) if name != "C" else (more, none) if lab[-1] == 1 else (none, more)
            q, t = cat(front, q, back), cat(front, t, back)
            qs, ts = qs + len(front), ts + len(front)
            assert 0 <= qs < len(q) and 0 <= ts < len(t)
            r = RC.letters(q.astype(np.uint8))
            reads.append(X.strand_letters(r, 1).copy() if jb[2] else r)
            names.append(b"t%d" % len(seqs))
            seqs.append(RC.letters(t.astype(np.uint8)))
            cands.append((len(reads) - 1, jb[2], at + ts + 1, qs, 7))
            starts.append(q)
            at += len(t)
        text = RC.fasta_bytes(names, seqs, width=60)
        codes, _ = XC.ref_codes(text)
        assert len(codes) == at
        walks = []
        for q, c in zip(starts, cands):
            ref_start, read_start, left, right = X.window(len(codes), len(q), c[2], c[3])
            w = walk(q, read_start, codes[ref_start - left: ref_start + right].astype(np.int8), left)
            w["sb"] = ref_start - left
            walks.append(w)
        _made[key] = dict(text=text, reads=reads, cands=np.array(cands, dtype=np.int64), walks=walks, codes=codes, labels=[p[4] for p in f.pairs[lo:hi]])
    return _made[key]
