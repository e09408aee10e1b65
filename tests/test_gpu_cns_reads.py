"""The corrected reads on the device (mecat_amd/csrc/cns_reads.hip; mhip_cns_accept_templates_reads, mhip_cns_format_reads,
mhip_debug_cns_reads, mhip_debug_cns_correct): the rest of consensus_worker behind the POA.  Expected values are the reference's own
records in tests/golden/cns_reads.npz where a case is in the fixture, otherwise the literal restatement tests/cns_reads_ref.py, which
test_cns_reads_ref_cpu.py holds to that fixture.  Everything goes through the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest

import cns_plan_ref as PR
import cns_poa_cases as P
import cns_reads_ref as R
import helpers as H

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(H.GOLDEN, "cns_accept.npz"))
FMAT, UNDS = 1, 8


@pytest.fixture(scope="module")
def ctx():
    import mecat_amd.hip as M
    c = M.Context(0)
    yield c
    c.close()


# ---- the kernel hook against the restatement ------------------------------------------------------------------------------------------

def synth_template(rng, L, segs):
    """a table with random letters, ident bytes and plan records from a description: segs = [(beg, end, anchors, {sb: string})] with
    anchors the FMAT positions and a listed window from each sb (an anchor) to the next anchor or the segment's end"""
    base = rng.choice(list(b"ACGT"), L).astype(np.uint8)
    ident = np.full(L, UNDS, np.uint8)
    out = []
    for beg, end, anchors, listed in segs:
        anchors = sorted(anchors)
        assert all(beg <= a < end for a in anchors) and set(listed) <= set(anchors)
        ident[anchors] = FMAT
        wins = []
        for a, nxt in zip(anchors, anchors[1:] + [end]):
            if a in listed:
                wins.append((a, nxt, 3, listed[a]))
        out.append((beg, end, len(anchors), wins))
    return base, ident, out


def hook(ctx, templates, min_size):
    """templates: [(base, ident, [(beg, end, n_anchors, [(sb, se, cov, string)])], read_id)] -> (the hook's dict, the restatement's reads
    and seq, read_begin)"""
    import mecat_amd.hip as M
    table = np.zeros(sum(len(t[0]) for t in templates), M.TABLE_DTYPE)
    table["base"] = np.concatenate([t[0] for t in templates])
    table["mat_cnt"] = 3
    ident = np.concatenate([t[1] for t in templates])
    tbeg = np.concatenate([[0], np.cumsum([len(t[0]) for t in templates])]).astype(np.int64)
    segs, wins, strings, recs, targets, rb = [], [], [], [], [], [0]
    for k, (base, idn, sg, rid) in enumerate(templates):
        s0 = len(segs)
        for beg, end, na, ws in sg:
            segs.append((k, beg, end, na, len(wins), len(wins) + len(ws)))
            wins += [(sb, se, cov, len(segs) - 1) for sb, se, cov, _ in ws]
            strings += [bytes(w[3]) for w in ws]
        sarr = np.array(segs[s0:], dtype=M.SEGMENT_DTYPE) if len(segs) > s0 else np.zeros(0, M.SEGMENT_DTYPE)
        warr = np.array(wins, dtype=M.WINDOW_DTYPE) if wins else np.zeros(0, M.WINDOW_DTYPE)
        r, t = R.reads_of(base.tolist(), idn.tolist(), sarr, warr, strings, min_size, rid, template_index=k, seg_base=s0)
        recs += [x[:7] + (x[7] + len(targets),) for x in r]
        targets += t
        rb.append(len(recs))
    want_reads, want_seq = R.as_arrays(recs, targets)
    cb = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    got = M.debug_cns_reads(ctx, table, ident, tbeg, [t[3] for t in templates], np.array(segs, dtype=M.SEGMENT_DTYPE) if segs else np.zeros(0, M.SEGMENT_DTYPE),
                            np.array(wins, dtype=M.WINDOW_DTYPE) if wins else np.zeros(0, M.WINDOW_DTYPE), np.frombuffer(b"".join(strings), dtype=np.uint8), cb, min_size)
    return got, want_reads, want_seq, np.array(rb, np.int64)


def check_hook(ctx, templates, min_size):
    got, reads, seq, rb = hook(ctx, templates, min_size)
    assert got["reads"].tobytes() == reads.tobytes(), (got["reads"][:4], reads[:4])
    assert got["seq"].tobytes() == seq.tobytes()
    assert np.array_equal(got["read_begin"], rb)
    return got


def test_hook_step_edges(ctx):
    rng = np.random.default_rng(41)
    letters = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    # anchors and windows at positions 63, 64 and 65 of a segment that begins at 5; window strings of 0, 1, 2, 3 and 1 500 letters
    S = [b"", letters(1), letters(2), letters(3), letters(1500)]
    for at in ([63], [64], [65], [63, 64, 65], [0, 63, 64, 65, 127, 128, 129]):
        anchors = sorted(set([5 + a for a in at] + [5 + 200, 5 + 201]))
        for k in range(len(S)):
            listed = {5 + a: S[(k + i) % len(S)] for i, a in enumerate(at)}
            t = synth_template(rng, 400, [(5, 300, anchors, listed)])
            got = check_hook(ctx, [t + (9,)], 2)
            assert len(got["reads"]) == 1
    # every position an anchor, every anchor with a window (64 windows begin in every step), strings of 0 .. 12 letters and some long ones
    anchors = list(range(10, 330))
    listed = {a: letters(int(rng.choice([0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 70, 700]))) for a in anchors}
    check_hook(ctx, [synth_template(rng, 340, [(10, 330, anchors, listed)]) + (1,)], 2)
    # a window spanning three 64-position steps; a segment whose first 70 positions hold no anchor; a last window that ends at the segment's end
    check_hook(ctx, [synth_template(rng, 400, [(0, 390, [3, 50, 260, 261], {50: letters(40), 261: letters(7)})]) + (2,)], 2)
    check_hook(ctx, [synth_template(rng, 400, [(7, 390, [77, 78, 300], {78: letters(5)})]) + (3,)], 2)
    got = check_hook(ctx, [synth_template(rng, 400, [(7, 390, [], {})]) + (4,)], 2)          # no anchor at all: no read
    assert len(got["reads"]) == 0 and len(got["seq"]) == 0 and got["read_begin"].tolist() == [0, 0]
    # two segments of one template and segments of neighbouring templates, one template without a segment between them
    a = synth_template(rng, 500, [(0, 200, list(range(0, 200, 3)), {6: letters(9), 198: letters(4)}), (250, 500, list(range(251, 500, 2)), {251: letters(3)})])
    b = synth_template(rng, 130, [])
    c = synth_template(rng, 260, [(1, 259, list(range(1, 259)), {64: letters(30), 65: letters(2), 258: letters(6)})])
    got = check_hook(ctx, [a + (11,), b + (12,), c + (13,)], 50)
    assert got["read_begin"].tolist() == [0, 2, 2, 3] and got["reads"]["read_id"].tolist() == [11, 11, 13] and got["reads"]["segment"].tolist() == [0, 1, 2]
    # targets of min_size - 1 and min_size letters: 40 anchors and a window that adds 9
    t = synth_template(rng, 100, [(10, 90, list(range(20, 60)), {30: letters(11)})])
    assert len(check_hook(ctx, [t + (5,)], 49)["reads"]) == 1 and len(check_hook(ctx, [t + (5,)], 50)["reads"]) == 0


@pytest.mark.parametrize("size", R.LONG_SIZES)
def test_hook_long_sizes(ctx, size):
    """the five sizes around the block rule on generated tables: every third position an anchor, windows that add the rest"""
    rng = np.random.default_rng(size)
    beg = 13
    n_anch = size // 2
    end = beg + 3 * n_anch
    anchors = list(range(beg, end, 3))
    extra = size - n_anch
    listed = {}
    for i, a in enumerate(anchors[:: 64]):
        n = min(extra, 700 if i % 7 == 0 else 150)
        extra -= n
        listed[a] = bytes(rng.choice(list(b"ACGT"), n + 2).astype(np.uint8))
    assert extra == 0
    got = check_hook(ctx, [synth_template(rng, end + 9, [(beg, end, anchors, listed)]) + (77,)], 5000)
    assert got["reads"]["size"].tolist() == [hi - lo for lo, hi, _, _ in R.split(size, beg, end)] and len(got["seq"]) == size


def test_hook_fixture_tables(ctx):
    """the hand-written fixture cases: the host back end's table, plan and window strings through the kernels"""
    import mecat_amd.hip as M
    cases, rows = R.load_fixture()
    n = 0
    for c, row in zip(cases, rows):
        if c["long"] is not None or c["read_id"] != 7:
            continue
        h = R.host_back_end(c)
        cb = np.concatenate([[0], np.cumsum([len(s) for s in h["strings"]])]).astype(np.int64)
        got = M.debug_cns_reads(ctx, h["table"], h["ident"], [0, len(c["tmpl"])], [c["read_id"]], h["plan"]["segments"], h["plan"]["windows"],
                                np.frombuffer(b"".join(h["strings"]), dtype=np.uint8), cb, c["min_size"])
        assert R.same_as_recorded(R.results_of(got["reads"], got["seq"]), row)
        n += 1
    assert n >= 15


# ---- the chain hook: every fixture case, byte-equal to what the reference recorded ----------------------------------------------------

def test_chain_fixture(ctx):
    import mecat_amd.hip as M
    cases, rows = R.load_fixture()
    nrec = 0
    for i, (c, row) in enumerate(zip(cases, rows)):
        buf, off, ln, soff, send = P.pack_alns(c["alns"])
        reads, seq = M.debug_cns_correct(ctx, buf, off, ln, soff, send, c["tmpl"], c["tech"], c["min_cov"], c["min_size"], c["read_id"])
        assert R.same_as_recorded(R.results_of(reads, seq), row), i
        nrec += len(row)
    assert nrec > 200


# ---- the whole call on the golden accept sets ----------------------------------------------------------------------------------------
_sets = {}


def golden_set(name, n):
    if (name, n) not in _sets:
        from mecat_amd import workload as W
        nr, L, Gn, seed, ont, tech, mas = (int(x) for x in G[name + "_par"])
        err, ratio = (float(x) for x in G[name + "_ratio"])
        codes, lens = W.synth_reads(nr, L, err, Gn, seed, ont)
        pac, offs, nb = W.pack_volume(codes, lens)
        tb = G[name + "_tmpl_begin"][: n + 1].copy()
        _sets[name, n] = dict(pac=pac, offs=offs, nb=nb, lens=lens, tb=tb, cands=G[name + "_cands"][: tb[n]].copy(), tech=tech, mas=mas, ratio=ratio)
    return _sets[name, n]


def run(ctx, g, want, entry="reads", tb=None, ratio=None, params=None):
    import mecat_amd.hip as M
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], 0)
    try:
        f = {"reads": M.cns_accept_templates_reads, "poa": M.cns_accept_templates_poa}[entry]
        out = f(ctx, vol, g["cands"].copy(), g["tb"] if tb is None else tb, g["tech"], g["mas"], g["ratio"] if ratio is None else ratio, want,
                *(params or PR.DEFAULTS[g["tech"]]), threads=16)
        cp = lambda x: np.array(x, copy=True) if isinstance(x, np.ndarray) else ({k: np.array(v, copy=True) for k, v in x.items()} if isinstance(x, dict) else x)
        return tuple(cp(x) for x in out)
    finally:
        vol.free()


def same_reads(x, y):
    return all(x[k].tobytes() == y[k].tobytes() for k in ("reads", "read_begin", "seq"))


def restated(g, out, tb, min_size):
    """the restatement applied to a call's own table, plan and cns -> (reads, seq, read_begin)"""
    table, ident, begin, plan = out[3], out[4], out[5], out[6]
    win, cb, cns = plan["windows"], plan["cns_begin"], plan["cns"].tobytes()
    strings = [cns[cb[w]: cb[w + 1]] for w in range(len(win))]
    recs, targets, rb = [], [], [0]          # (a candidate record is 13 int32, sid the eighth: mhip_ext_candidate)
    for t in range(len(tb) - 1):
        s0, s1 = plan["seg_begin"][t: t + 2]
        if s1 > s0:
            tab = table[begin[t]: begin[t + 1]]
            r, tg = R.reads_of(tab["base"].tolist(), ident[begin[t]: begin[t + 1]].tolist(), plan["segments"][s0: s1], win, strings, min_size,
                               int(np.asarray(g["cands"]).reshape(-1, 13)[tb[t], 7]), template_index=t, seg_base=int(s0))
            recs += [x[:7] + (x[7] + len(targets),) for x in r]
            targets += tg
        rb.append(len(recs))
    reads, seq = R.as_arrays(recs, targets)
    return reads, seq, np.array(rb, np.int64)


@pytest.mark.parametrize("name,n,params", [("pacbio", 48, (4, 3000)), ("pacbio", 24, None), ("nanopore", 32, None), ("nanopore", 24, (4, 3000))])
def test_whole_call(ctx, name, n, params):
    import mecat_amd.hip as M
    S, TB, PL, PC, PO, RD = M.CNS_WANT_STRINGS, M.CNS_WANT_TABLE, M.CNS_WANT_PLAN, M.CNS_WANT_PIECES, M.CNS_WANT_POA, M.CNS_WANT_READS
    g = golden_set(name, n)
    min_size = (params or PR.DEFAULTS[g["tech"]])[1]
    full = run(ctx, g, S | TB | PL | PC | PO | RD, params=params)
    reads, seq, rb = restated(g, full, g["tb"], min_size)
    got = full[7]
    print(name, n, params, "reads", len(got["reads"]), "letters", len(got["seq"]), "segments", len(full[6]["segments"]))
    assert got["reads"].tobytes() == reads.tobytes() and got["seq"].tobytes() == seq.tobytes() and np.array_equal(got["read_begin"], rb)
    if name == "pacbio" and params is not None:
        assert len(reads) >= 5 and len(seq) >= 5 * min_size
    # everything else is what _poa returns; without the bit the call is _poa
    ref = run(ctx, g, S | TB | PL | PC | PO, entry="poa", params=params)
    none = run(ctx, g, S | TB | PL | PC | PO, params=params)
    assert none[7] is None
    for x in (full, none):
        assert x[2] == ref[2] and all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x[:2] + x[3:6], ref[:2] + ref[3:6]))
        assert sorted(x[6]) == sorted(ref[6]) and all(x[6][k].tobytes() == ref[6][k].tobytes() for k in ref[6])
    # READS alone: the same reads, and no strings, tables, plan records, pieces or cns
    acc, s, nj, tab, idn, begin, plan, rd = run(ctx, g, RD, params=params)
    assert same_reads(rd, got) and plan is None and len(s) == 0 and len(tab) == 0 and len(idn) == 0 and len(begin) == 0
    assert acc.tobytes() == run(ctx, g, PL | PO, entry="poa", params=params)[0].tobytes() and np.all(acc["str_offset"] == -1)
    # READS with some of the other bits
    for w in (RD | PL, RD | TB, RD | PL | PO):
        x = run(ctx, g, w, params=params)
        assert same_reads(x[7], got) and (x[6] is None) == (not w & PL) and (len(x[3]) > 0) == bool(w & TB)
        if w & PL:
            assert PR.same_plan(x[6], full[6]) is None and ("cns" in x[6]) == bool(w & PO) and "pieces" not in x[6]
    # the text
    want_text = R.format_reads(reads, seq)
    assert M.cns_format_reads(got["reads"], got["seq"]) == want_text and (len(reads) == 0 or want_text.startswith(b">%d_" % reads[0]["read_id"]))


def test_slices_and_templates_without_work(ctx, monkeypatch):
    import mecat_amd.hip as M
    RD, PL, PO, S, TB, PC = M.CNS_WANT_READS, M.CNS_WANT_PLAN, M.CNS_WANT_POA, M.CNS_WANT_STRINGS, M.CNS_WANT_TABLE, M.CNS_WANT_PIECES
    g = golden_set("pacbio", 48)
    params = (4, 3000)
    one = run(ctx, g, RD, params=params)[7]
    assert len(one["reads"]) >= 5
    tb = np.concatenate([g["tb"][:21], g["tb"][20:]])          # a template without candidates in the middle of the batch
    mid = run(ctx, g, RD, tb=tb, params=params)[7]
    shifted = one["reads"].copy()
    shifted["template_index"] += shifted["template_index"] >= 20
    assert mid["reads"].tobytes() == shifted.tobytes() and mid["seq"].tobytes() == one["seq"].tobytes()
    assert np.array_equal(mid["read_begin"], np.concatenate([one["read_begin"][:21], one["read_begin"][20:]]))
    monkeypatch.setenv("MECAT_CNS_SLICE_JOBS", "1500")          # >= 3 slices: both scratch sets are used again
    for w in (RD, RD | S | TB | PL | PC | PO):
        many = run(ctx, g, w, params=params)
        assert many[2] > 2 * 1500 and same_reads(many[7], one)
        assert same_reads(run(ctx, g, w, tb=tb, params=params)[7], mid)
    # every template a slice of its own, some without a segment, one without candidates
    g12 = golden_set("pacbio", 12)
    tb12 = np.concatenate([g12["tb"][:7], g12["tb"][6:]])
    kw = dict(tb=tb12, ratio=1.0, params=params)
    monkeypatch.delenv("MECAT_CNS_SLICE_JOBS")
    whole = {w: run(ctx, g12, w, **kw) for w in (RD, RD | PL | PO)}
    assert len(whole[RD][7]["reads"]) >= 1
    monkeypatch.setenv("MECAT_CNS_SLICE_JOBS", "1")
    for w, x in whole.items():
        y = run(ctx, g12, w, **kw)
        assert same_reads(x[7], y[7]) and x[0].tobytes() == y[0].tobytes()
        if w & PL:
            assert all(x[6][k].tobytes() == y[6][k].tobytes() for k in x[6])
    monkeypatch.delenv("MECAT_CNS_SLICE_JOBS")
    # nothing accepted: no read, read_begin all zero
    acc, _, nj, _, _, _, _, rd = run(ctx, golden_set("pacbio", 4), RD, ratio=1.52)
    assert len(acc) == 0 and nj > 0 and len(rd["reads"]) == 0 and len(rd["seq"]) == 0 and rd["read_begin"].tolist() == [0] * 5
    assert M.cns_format_reads(rd["reads"], rd["seq"]) == b""


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def raw_reads_call(ctx, g, want, missing):
    """mhip_cns_accept_templates_reads with one of its four last output pointers NULL"""
    import mecat_amd.hip as M
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], 0)
    try:
        cands, tb = g["cands"].copy(), np.ascontiguousarray(g["tb"], dtype=np.int64)
        vp = [C.c_void_p() for _ in range(17)]
        i64 = [C.c_int64() for _ in range(5)]
        outs = [vp[0], i64[0], vp[1], i64[1], i64[2], vp[2], vp[3], vp[4], vp[5], vp[6], vp[7], i64[3], vp[8], vp[9], vp[10], vp[11], vp[12], vp[13], vp[14], vp[15], vp[16], i64[4]]
        refs = [C.byref(o) for o in outs]
        refs[len(refs) - 4 + missing] = None
        rc = M.lib().mhip_cns_accept_templates_reads(ctx.h, vol.h, cands.ctypes.data, tb.ctypes.data, len(tb) - 1, g["tech"], g["mas"], float(g["ratio"]), 4, want, 4, 3000, *refs)
        if rc:
            raise M.MhipError(M.lib().mhip_last_error().decode())
        for p in vp:
            M.lib().mhip_cns_free(p)
    finally:
        vol.free()


def test_refusals(ctx):
    import mecat_amd.hip as M
    S, TB, PL, PC, PO, RD = M.CNS_WANT_STRINGS, M.CNS_WANT_TABLE, M.CNS_WANT_PLAN, M.CNS_WANT_PIECES, M.CNS_WANT_POA, M.CNS_WANT_READS
    g = golden_set("pacbio", 4)
    for want in (0, 64, RD | 64, RD | 128, -1, RD | PC, RD | PO, RD | PC | PO | S, PO, PC | TB):          # unknown bits; PIECES or POA without PLAN
        with pytest.raises(M.MhipError, match="want"):
            run(ctx, g, want)
    for missing in range(4):
        with pytest.raises(M.MhipError, match="reads were asked for without a place"):
            raw_reads_call(ctx, g, RD, missing)
    raw_reads_call(ctx, g, PL, 0)                               # without the bit the pointers may be NULL
    with pytest.raises(M.MhipError, match="min_size"):
        run(ctx, g, RD, params=(4, 1))
    # the read hook
    rng = np.random.default_rng(3)
    t = synth_template(rng, 200, [(10, 150, [20, 30, 40], {20: b"ACGT", 40: b"AAAAA"})])
    good = lambda: ([np.array(x) for x in (t[0], t[1])], [list(s[:3]) + [[list(w[:3]) for w in s[3]]] for s in t[2]])

    def call(mut, min_size=2, strings=None, cb=None, tbeg=None):
        (base, ident), segs = good()
        table = np.zeros(len(base), M.TABLE_DTYPE)
        table["base"] = base
        seg = np.array([(0, s[0], s[1], s[2], 0, len(s[3])) for s in segs], dtype=M.SEGMENT_DTYPE)
        win = np.array([(w[0], w[1], w[2], 0) for s in segs for w in s[3]], dtype=M.WINDOW_DTYPE)
        mut(seg, win)
        strings = [b"ACGT", b"AAAAA"] if strings is None else strings
        cb = np.concatenate([[0], np.cumsum([len(s) for s in strings])]) if cb is None else cb
        return M.debug_cns_reads(ctx, table, ident, [0, len(base)] if tbeg is None else tbeg, [1], seg, win, np.frombuffer(b"".join(strings), dtype=np.uint8), cb, min_size)

    assert len(call(lambda s, w: None)["reads"]) == 1

    def setf(arr, i, k, v):
        arr[k][i] = v

    for mut, match in ((lambda s, w: setf(w, 1, "sb", 25), "ascending and disjoint"), (lambda s, w: setf(w, 0, "se", 45), "ascending and disjoint"),
                       (lambda s, w: setf(w, 1, "se", 151), "outside its segment"), (lambda s, w: setf(w, 0, "sb", 9), "outside its segment"),
                       (lambda s, w: setf(w, 0, "se", 20), "sb < se"), (lambda s, w: setf(w, 1, "segment", 1), "outside its segment"),
                       (lambda s, w: setf(s, 0, "end", 201), "outside its template"), (lambda s, w: setf(s, 0, "beg", -1), "outside its template"),
                       (lambda s, w: setf(s, 0, "template_index", 1), "template order"), (lambda s, w: setf(s, 0, "win_end", 3), "inside the list"),
                       (lambda s, w: setf(s, 0, "win_begin", 3), "win_begin <= win_end")):
        with pytest.raises(M.MhipError, match=match):
            call(mut)
    with pytest.raises(M.MhipError, match="does not ascend"):
        call(lambda s, w: None, cb=np.array([0, 5, 4]))
    with pytest.raises(M.MhipError, match="start at 0"):
        call(lambda s, w: None, cb=np.array([1, 5, 9]))
    with pytest.raises(M.MhipError, match="min_size"):
        call(lambda s, w: None, min_size=1)
    # what only the kernels see: a window that does not begin on an anchor, an n_anchors that is not the segment's -> refused, not truncated
    with pytest.raises(M.MhipError, match="letters written are not the letters counted"):
        call(lambda s, w: setf(w, 0, "sb", 21))
    with pytest.raises(M.MhipError, match="letters written are not the letters counted"):
        call(lambda s, w: setf(s, 0, "n_anchors", 4))
    with pytest.raises(M.MhipError, match="letters written are not the letters counted"):
        call(lambda s, w: setf(s, 0, "n_anchors", 2))
    # the chain hook: what the table and piece hooks refuse
    tm = b"ACGTA" * 10

    def chain(alns, tmpl=tm, min_cov=1, min_size=2):
        buf, off, ln, soff, send = P.pack_alns(alns)
        return M.debug_cns_correct(ctx, buf, off, ln, soff, send, tmpl, 1, min_cov, min_size, 5)

    ok = (tm[10: 15], tm[10: 15], 10, 15)
    assert len(chain([ok] * 3)[0]) == 1
    for alns, kw, match in (([(b"AGGTA", b"ACGTA", 10, 15)], {}, "mismatch"), ([(tm[:5], tm[:5], 48, 53)], {}, "leaves the template"), ([ok] * 101, {}, "100"),
                            ([(b"", b"", 3, 3)], {}, "len"), ([(tm[:5], tm[:5], 10, 16)], {}, "send - soff"), ([(tm[:5], tm[:5], -1, 4)], {}, "negative"),
                            ([ok], dict(min_size=1), "min_size"), ([ok], dict(min_cov=0), "min_cov")):
        with pytest.raises(M.MhipError, match=match):
            chain(alns, **kw)
    assert len(chain([])[0]) == 0
    # the text: a record that leaves the letters
    bad = np.zeros(1, M.READ_DTYPE)
    bad["size"], bad["seq_begin"] = 5, 2
    with pytest.raises(M.MhipError, match="leaves the letters"):
        M.cns_format_reads(bad, np.zeros(6, np.uint8))
