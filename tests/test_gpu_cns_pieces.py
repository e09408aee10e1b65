"""The POA windows' substrings on the device (mecat_amd/csrc/cns_pieces.hip; mhip_cns_accept_templates_pieces, mhip_debug_cns_pieces):
CnsAln::retrieve_aln_subseqs (mecat2cns/reads_correction_aux.h:47-68) for every listed window and every accepted alignment, as
descriptors.  Every case compares bytes with the literal cursor of tests/cns_pieces_ref.py (held against hand-computed pieces and
against the closed form in test_cns_pieces_ref_cpu.py); the strings and the plan the pipeline cases start from are pinned by
test_gpu_cns_accept.py / test_gpu_cns_plan.py.  Everything goes through the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest

import cns_pieces_cases as K
import cns_pieces_ref as Q
import cns_plan_ref as P
import helpers as H

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(H.GOLDEN, "cns_accept.npz"))


@pytest.fixture(scope="module")
def ctx():
    import mecat_amd.hip as M
    c = M.Context(0)
    yield c
    c.close()


def pack(alns):
    """alignments -> the hook's arguments (buf, off, len, soff, send): qaln + NUL, saln + NUL, pair after pair"""
    buf, off = bytearray(b"\0" * 3), []                     # (the first pair does not start at 0)
    for q, s, soff, send in alns:
        off.append(len(buf))
        buf += bytes(q) + b"\0" + bytes(s) + b"\0"
    return (np.frombuffer(bytes(buf), np.uint8), np.array(off, np.int64), np.array([len(a[1]) for a in alns], np.int32), np.array([a[2] for a in alns], np.int32),
            np.array([a[3] for a in alns], np.int32))


def hook(ctx, alns, windows):
    import mecat_amd.hip as M
    return M.debug_cns_pieces(ctx, *pack(alns), np.asarray(windows, np.int32).reshape(-1, 2))


def check(ctx, alns, windows):
    got = hook(ctx, alns, windows)
    want = Q.retrieve_literal(alns, windows)
    assert Q.same_pieces(got, want) is None, (Q.same_pieces(got, want), windows)
    return got


def test_hook_hand_computed(ctx):
    for name, (alns, windows, pieces, piece_begin) in sorted(K.HAND.items()):
        got = check(ctx, alns, windows)
        assert Q.same_pieces(got, Q.as_arrays(pieces, piece_begin)) is None, name


def test_hook_step_edges(ctx):
    """alignments of 63 .. 129 columns, one step of 64 columns after the other; window boundaries on columns 63 | 64 and 127 | 128; gap
    runs across a step boundary; a window over three steps"""
    rng = np.random.default_rng(7)
    letters = lambda n: "".join(rng.choice(list("ACGT"), n))
    alns = [K.aln(letters(n), 5) for n in (63, 64, 65, 127, 128, 129)]                      # column c at position 5 + c
    alns.append(K.aln(letters(60) + "-" * 11 + letters(140), 5))                           # a gap run over columns 60 .. 70
    alns.append(K.aln(letters(64) + "-" * 64 + letters(10), 5))                            # a whole step of gaps: columns 64 .. 127
    alns.append(K.aln("-" + letters(62) + "-" + letters(66), 5))                           # saln[0] a gap, a gap on column 63
    alns.append(K.aln(letters(200), 0))
    alns.append(K.aln(letters(126) + "---", 5))                                            # trailing gaps up to column 128
    boundaries = [(5 + 60, 5 + 63), (5 + 63, 5 + 64), (5 + 64, 5 + 65), (5 + 65, 5 + 70), (5 + 120, 5 + 127), (5 + 127, 5 + 128), (5 + 128, 5 + 131)]
    got = check(ctx, alns, boundaries)
    assert got[0][got[1][1]: got[1][2]][["aln", "col", "ncols"]].tolist()[:3] == [(2, 63, 2), (3, 63, 2), (4, 63, 2)]      # by hand, window (68, 69): 63 columns end in front of it, 64 are spent by (65, 68)
    check(ctx, alns, [(5 + 10, 5 + 180)])                                                  # a window over three steps
    check(ctx, alns, [(0, 5 + 63), (5 + 64, 5 + 127), (5 + 127, 5 + 128), (5 + 128, 400)])
    check(ctx, alns, [(p, p + 1) for p in range(0, 210)])                                  # a window per position, touching
    check(ctx, alns, [(p, p + 1) for p in range(1, 210, 2)])
    for name, (a, w, _, _) in sorted(K.HAND.items()):                                      # the CPU cases moved behind a step boundary
        if a:
            pre = letters(70)                                                              # column 0 becomes column 70, every position moves by 100
            check(ctx, [K.aln(pre + s.decode(), soff + 30, pre + q.decode()) for q, s, soff, send in a], [(sb + 100, se + 100) for sb, se in w])


def test_hook_width(ctx):
    """100 alignments on one window: both ballot rounds, the 64th and the 65th alignment the only ones with a part of it"""
    out = [K.aln("ACGTACGT", 60), K.aln("ACGTACGT", 42), K.aln("A", 52)]                    # se <= soff; send <= sb; n == 1
    alns = [out[k % 3] for k in range(100)]
    alns[63] = K.aln("ACGTACGTACGTACGTACGTACGTACGTACGT", 40)
    alns[64] = K.aln("ACGTAC-GT", 52)
    got = check(ctx, alns, [(50, 60)])
    assert got[0].tolist() == [(63, 10, 11, 50), (64, 0, 9, 52)] and got[1].tolist() == [0, 2]
    got = check(ctx, [alns[63]] * 100, [(41, 50), (50, 60), (60, 90)])
    assert np.array_equal(got[0]["aln"], np.tile(np.arange(100), 3)) and got[1].tolist() == [0, 100, 200, 300]
    import mecat_amd.hip as M
    with pytest.raises(M.MhipError, match="100"):
        hook(ctx, alns + [alns[0]], [(50, 60)])


@pytest.mark.parametrize("nwin", [1023, 1024, 1025, 2049])
def test_hook_window_counts_across_the_scan_tiles(ctx, nwin):
    """cns_pieces_scan turns the windows' piece counts into piece_begin, 1 024 windows a tile with a running sum: window lists that end
    one short of a tile, on it, one behind it and one behind the second — a window on every other position, three alignments that each
    cover a part of the template, so the counts are 1 .. 3 and change along the list"""
    rng = np.random.default_rng(nwin)
    letters = lambda n: "".join(rng.choice(list("ACGT"), n))
    L = 2 * nwin + 1
    alns = [K.aln(letters(L), 0), K.aln(letters(L - 700), 300), K.aln(letters(500) + "--" + letters(900), 1100)]
    got = check(ctx, alns, [(2 * w, 2 * w + 1) for w in range(nwin)])
    cnt = np.diff(got[1])
    assert len(cnt) == nwin and cnt.min() >= 1 and cnt.max() == 3 and got[1][-1] == len(got[0]) > nwin


def test_hook_random(ctx):
    """250 seeded templates of up to 2 000 positions and up to 40 alignments, gap runs of up to 70 columns, random window lists"""
    rng = np.random.default_rng(20262)
    count = dict.fromkeys(K.SITUATIONS, 0)
    npieces = 0
    for case in range(250):
        L = int(rng.choice([40, 150, 700, 2000]))
        alns, windows = K.random_case(rng, L, int(rng.choice([3, 12, 40])), int(rng.choice([30, 150, 600])) if L > 40 else 30)
        got = check(ctx, alns, windows)
        K.census(alns, windows, got[0], got[1], count)
        npieces += len(got[0])
    assert npieces >= 250 * 20 and all(count[k] >= 5 for k in K.SITUATIONS), (npieces, count)


# ---- the pipeline on the golden accept sets ------------------------------------------------------------------------------------------
FULL = {"pacbio": 240, "nanopore": 160}
CHUNK = 30                # templates per case of the literal comparison: the cursor walks 0.15 M columns per template in Python
_sets, _runs = {}, {}


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


def run(ctx, g, want, pieces=True, tb=None, ratio=None, params=None):
    """mhip_cns_accept_templates_pieces (pieces=False: mhip_cns_accept_templates_plan) -> its tuple, arrays copied"""
    import mecat_amd.hip as M
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], 0)
    try:
        f = M.cns_accept_templates_pieces if pieces else M.cns_accept_templates_plan
        out = f(ctx, vol, g["cands"].copy(), g["tb"] if tb is None else tb, g["tech"], g["mas"], g["ratio"] if ratio is None else ratio, want,
                *(params or P.DEFAULTS[g["tech"]]), threads=16)
        cp = lambda x: np.array(x, copy=True) if isinstance(x, np.ndarray) else ({k: np.array(v, copy=True) for k, v in x.items()} if isinstance(x, dict) else x)
        return tuple(cp(x) for x in out)
    finally:
        vol.free()


def full_run(ctx, name, want, pieces=True):
    """the whole golden set at the defaults, run once per mode and shared (read-only)"""
    if (name, want, pieces) not in _runs:
        _runs[name, want, pieces] = run(ctx, golden_set(name, FULL[name]), want, pieces)
    return _runs[name, want, pieces]


def template_input(acc, strings, plan, first, t):
    """template t of a call's output -> (alignments from the call's own strings, windows from its own plan, first window)"""
    alns = []
    for r in acc[first[t]: first[t + 1]]:
        o, n = int(r["str_offset"]), int(r["aln_size"])
        alns.append((strings[o: o + n].tobytes(), strings[o + n + 1: o + 2 * n + 1].tobytes(), int(r["soff"]), int(r["send"])))
    s0, s1 = int(plan["seg_begin"][t]), int(plan["seg_begin"][t + 1])
    w0 = int(plan["segments"]["win_begin"][s0]) if s1 > s0 else 0
    w1 = int(plan["segments"]["win_end"][s1 - 1]) if s1 > s0 else 0
    return alns, [(int(w["sb"]), int(w["se"])) for w in plan["windows"][w0: w1]], w0


def pieces_of(plan, w0, nw, aln0):
    """the pieces of windows [w0, w0 + nw) with `aln` and piece_begin counted from the template's first"""
    pb = plan["piece_begin"][w0: w0 + nw + 1]
    pc = plan["pieces"][pb[0]: pb[-1]].copy()
    pc["aln"] -= aln0
    return pc, pb - pb[0]


ALL_MODES = 1 | 4 | 8         # STRINGS | PLAN | PIECES


@pytest.mark.parametrize("name,chunk", [(n, c) for n in sorted(FULL) for c in range((FULL[n] + CHUNK - 1) // CHUNK)])
def test_pipeline_pieces_are_the_literal_cursor(ctx, name, chunk):
    """every template: the literal cursor over the call's own strings and plan"""
    acc, strings, nj, _, _, _, plan = full_run(ctx, name, ALL_MODES)
    n = FULL[name]
    first = np.concatenate([[0], np.cumsum(np.bincount(acc["template_index"], minlength=n))])
    assert len(plan["piece_begin"]) == len(plan["windows"]) + 1 and plan["piece_begin"][0] == 0 and plan["piece_begin"][-1] == len(plan["pieces"])
    for t in range(chunk * CHUNK, min(n, (chunk + 1) * CHUNK)):
        alns, windows, w0 = template_input(acc, strings, plan, first, t)
        got = pieces_of(plan, w0, len(windows), first[t])
        want = Q.retrieve_literal(alns, windows)
        assert Q.same_pieces(got, want) is None, (t, Q.same_pieces(got, want))


@pytest.mark.parametrize("name", sorted(FULL))
def test_pipeline_modes(ctx, name):
    import mecat_amd.hip as M
    S, TB, PL, PC = M.CNS_WANT_STRINGS, M.CNS_WANT_TABLE, M.CNS_WANT_PLAN, M.CNS_WANT_PIECES
    full = full_run(ctx, name, S | PL | PC)
    # PLAN | PIECES: the same pieces and plan, and neither strings nor tables come back
    a, s, nj, tab, idn, begin, plan = full_run(ctx, name, PL | PC)
    assert len(s) == 0 and len(tab) == 0 and len(idn) == 0 and len(begin) == 0 and np.all(a["str_offset"] == -1)
    assert P.same_plan(plan, full[6]) is None and Q.same_pieces((plan["pieces"], plan["piece_begin"]), (full[6]["pieces"], full[6]["piece_begin"])) is None
    # without PIECES: mhip_cns_accept_templates_plan's output, byte for byte
    for want in (PL, S | TB | PL):
        x, y = run(ctx, golden_set(name, FULL[name]), want), full_run(ctx, name, want, pieces=False)
        assert "pieces" not in x[6] and all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x[:6], y[:6])) and x[2] == y[2]
        assert P.same_plan(x[6], y[6]) is None
    # the same bytes on a second run
    again = run(ctx, golden_set(name, FULL[name]), PL | PC)[6]
    assert again["pieces"].tobytes() == plan["pieces"].tobytes() and np.array_equal(again["piece_begin"], plan["piece_begin"])
    # the hook on a template's accepted strings and windows gives the pipeline's pieces (the first 8 templates)
    acc, strings, plan = full[0], full[1], full[6]
    first = np.concatenate([[0], np.cumsum(np.bincount(acc["template_index"], minlength=FULL[name]))])
    for t in range(8):
        alns, windows, w0 = template_input(acc, strings, plan, first, t)
        assert Q.same_pieces(hook(ctx, alns, windows), pieces_of(plan, w0, len(windows), first[t])) is None, t


def test_the_golden_sets_test_something(ctx):
    for name in sorted(FULL):
        acc, _, _, _, _, _, plan = full_run(ctx, name, ALL_MODES)
        pc, pb, win = plan["pieces"], plan["piece_begin"], plan["windows"]
        assert len(win) > 1000 and len(pc) >= 3 * len(win), (name, len(pc), len(win))      # >= min_cov alignments cover sb; only a spent one drops out
        w_of = np.repeat(np.arange(len(win)), np.diff(pb))
        assert np.all(np.diff(pc["aln"])[w_of[1:] == w_of[:-1]] > 0)                       # add order inside a window
        a = acc[pc["aln"]]
        assert (pc["sb_out"] > win["sb"][w_of]).any(), name                                # an alignment that starts inside a window
        assert ((pc["col"] + pc["ncols"] == a["aln_size"]) & (a["send"] <= win["se"][w_of])).any(), name      # ... and one that ends in one: clipped at n - 1


def test_slices_and_templates_without_work(ctx, monkeypatch):
    import mecat_amd.hip as M
    g = golden_set("pacbio", 48)
    params = (4, 3000)
    want = M.CNS_WANT_PLAN | M.CNS_WANT_PIECES
    one = run(ctx, g, want, params=params)[6]
    assert len(one["windows"]) > 1000 and len(one["pieces"]) >= 3 * len(one["windows"])
    monkeypatch.setenv("MECAT_CNS_SLICE_JOBS", "1500")          # >= 3 slices: both scratch sets are used again, the slices' pieces are put together
    for w in (want, want | M.CNS_WANT_STRINGS | M.CNS_WANT_TABLE):
        many = run(ctx, g, w, params=params)
        assert many[2] > 2 * 1500 and P.same_plan(one, many[6]) is None
        assert Q.same_pieces((many[6]["pieces"], many[6]["piece_begin"]), (one["pieces"], one["piece_begin"])) is None
    # a template without candidates in the middle of the batch, in slices and in one piece: the alignments behind it keep their numbers
    tb = np.concatenate([g["tb"][:21], g["tb"][20:]])
    for sliced in (True, False):
        if not sliced:
            monkeypatch.delenv("MECAT_CNS_SLICE_JOBS")
        p = run(ctx, g, want, tb=tb, params=params)[6]
        assert p["windows"].tobytes() == one["windows"].tobytes()
        assert Q.same_pieces((p["pieces"], p["piece_begin"]), (one["pieces"], one["piece_begin"])) is None
    # nothing accepted: no window, no piece
    for name in sorted(FULL):
        acc, _, nj, _, _, _, p = run(ctx, golden_set(name, 4), want, ratio=1.52)
        assert len(acc) == 0 and nj > 0 and len(p["windows"]) == 0 and len(p["pieces"]) == 0 and p["piece_begin"].tolist() == [0]


def test_refusals(ctx):
    import mecat_amd.hip as M
    g = golden_set("pacbio", 4)
    for want in (M.CNS_WANT_PIECES, M.CNS_WANT_PIECES | M.CNS_WANT_STRINGS, M.CNS_WANT_PIECES | M.CNS_WANT_TABLE, 0, 16, M.CNS_WANT_PLAN | M.CNS_WANT_PIECES | 16, -1):
        with pytest.raises(M.MhipError, match="want"):
            run(ctx, g, want)
    with pytest.raises(M.MhipError, match="want"):
        run(ctx, g, M.CNS_WANT_PLAN | M.CNS_WANT_PIECES, pieces=False)                     # mhip_cns_accept_templates_plan keeps refusing the bit
    # PIECES without a place to put them: the C entry point itself
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], 0)
    try:
        cands, tb = g["cands"].copy(), np.ascontiguousarray(g["tb"], dtype=np.int64)
        o = [C.c_void_p() for _ in range(10)]
        na, sb, nj, nwin = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        rc = M.lib().mhip_cns_accept_templates_pieces(ctx.h, vol.h, cands.ctypes.data, tb.ctypes.data, len(tb) - 1, g["tech"], g["mas"], g["ratio"], 4,
                                                      M.CNS_WANT_PLAN | M.CNS_WANT_PIECES, 4, 5000, C.byref(o[0]), C.byref(na), C.byref(o[1]), C.byref(sb), C.byref(nj),
                                                      C.byref(o[2]), C.byref(o[3]), C.byref(o[4]), C.byref(o[5]), C.byref(o[6]), C.byref(o[7]), C.byref(nwin), C.byref(o[8]),
                                                      C.byref(o[9]), None, None)
        assert rc != 0 and b"pieces" in M.lib().mhip_last_error() and not o[0].value and not o[7].value
    finally:
        vol.free()
    # the hook's input checks
    five, gap0 = K.FIVE, K.aln("-AC", 4)
    bad = lambda a, **kw: tuple(kw.get(k, v) for k, v in zip(("q", "s", "soff", "send"), a))
    for alns, windows, match in (([bad(five, send=16)], [(1, 2)], "bases"), ([bad(five, send=14)], [(1, 2)], "bases"), ([bad(gap0, send=7)], [(1, 2)], "bases"),
                                 ([bad(five, soff=-1, send=4)], [(1, 2)], "negative"), ([(b"", b"", 3, 3)], [(1, 2)], "len"), ([five], [(2, 2)], "sb < se"),
                                 ([five], [(3, 2)], "sb < se"), ([five], [(5, 8), (1, 3)], "ascending"), ([five], [(1, 5), (4, 8)], "disjoint"),
                                 ([five], [(-1, 3)], "negative")):
        with pytest.raises(M.MhipError, match=match):
            hook(ctx, alns, windows)
    buf, off, lens, soff, send = pack([five])
    with pytest.raises(M.MhipError, match="outside"):
        M.debug_cns_pieces(ctx, buf[:-2], off, lens, soff, send, [(1, 2)])
    assert hook(ctx, [gap0], [(4, 6)])[0].tolist() == [(0, 0, 3, 4)]                        # (send - soff counts saln[0] only when it is a base)
