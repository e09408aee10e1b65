"""The POA consensus of the listed windows on the device (mecat_amd/csrc/cns_poa.hip; mhip_cns_accept_templates_poa, mhip_debug_cns_poa):
meap_cns_one_indel (mecat2cns/mecat_correction.cpp:62-78) for every window.  Expected values are the reference's own strings recorded in
tests/golden/cns_poa.npz where a case is in the fixture, otherwise those of libcns_poa_host.so — the same routine (csrc/cns_poa.h)
compiled for the host, which test_cns_poa_ref_cpu.py pins to the compiled reference.  Everything goes through the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest

import cns_pieces_cases as K
import cns_pieces_ref as Q
import cns_plan_ref as PR
import cns_poa_cases as P
import helpers as H

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(H.GOLDEN, "cns_accept.npz"))


@pytest.fixture(scope="module")
def ctx():
    import mecat_amd.hip as M
    c = M.Context(0)
    yield c
    c.close()


def hook(ctx, alns, windows):
    """-> the windows' strings as a list of bytes"""
    import mecat_amd.hip as M
    buf, off, ln, soff, send = P.pack_alns(alns)
    cns, cb = M.debug_cns_poa(ctx, buf, off, ln, soff, send, np.asarray(windows, np.int32).reshape(-1, 3))
    assert len(cb) == len(windows) + 1 and cb[0] == 0 and cb[-1] == len(cns) and np.all(np.diff(cb) >= 0)
    return [cns[cb[w]: cb[w + 1]].tobytes() for w in range(len(windows))]


def last_launch():
    """(windows that went to cns_poa_large, launches of it) of the last POA launch"""
    import mecat_amd.hip as M
    o = (C.c_int64 * 2)()
    M.lib().mhip_debug_cns_poa_last(o)
    return int(o[0]), int(o[1])


def check(ctx, alns, windows):
    """the hook against the host routine -> (strings, info of the host routine)"""
    c = P.case(alns, windows)
    want, info = P.host_run(c)
    got = hook(ctx, alns, windows)
    assert got == want, [(w, g, x) for w, g, x in zip(windows, got, want) if g != x][:3]
    return got, info


def test_hook_fixture(ctx):
    """every fixture case, byte-equal to the strings the reference returned (the threshold cases window by window: fresh cursors)"""
    cases, strings = P.load_fixture()
    nwin = 0
    for i, (c, want) in enumerate(zip(cases, strings)):
        if c["fresh"]:
            got = [hook(ctx, c["alns"], [w])[0] for w in c["windows"]]
        else:
            got = hook(ctx, c["alns"], c["windows"])
        assert got == want, (i, [(w, g, x) for w, g, x in zip(c["windows"], got, want) if g != x][:3])
        nwin += len(want)
    assert nwin > 5000


def words_of(info):
    col = {n: i for i, n in enumerate(P.INFO_NAMES)}
    return [int(P.host_lib().cns_poa_host_words(int(r[col["bound_nodes"]]), int(r[col["bound_edges"]]))) for r in info]


def window_of_words(target, at):
    """alignments and one window (at, at + blen - 1) whose workspace bound is exactly `target` words: k alignments over the whole window,
    S insertion columns and D query gaps among them.  words = 17 (blen + 2 + S) + 8 (blen + 1 + k (blen + 1) - D + S)"""
    for blen in range(59, 5, -1):
        for S in range(0, 8):
            rem = target - 42 - 25 * blen - 25 * S
            if rem <= 0 or rem % 8:
                continue
            e = rem // 8
            k = -(-e // (blen + 1))
            D = k * (blen + 1) - e
            if k < 1 or k > 100 or D > k * (blen - 2) or S > k:
                continue
            alns = []
            for a in range(k):
                d = min(D, blen - 2)
                D -= d
                s = "A" + ("-" if a < S else "") + "C" * d + "G" * (blen - 1 - d)
                q = "A" + ("T" if a < S else "") + "-" * d + "G" * (blen - 1 - d)
                alns.append(K.aln(s, at, q))
            return alns, (at, at + blen - 1, k)
    raise AssertionError("no window of %d words" % target)


def test_lane_and_launch_edges(ctx, monkeypatch):
    import mecat_amd.hip as M
    rng = np.random.default_rng(11)
    letters = lambda n: "".join(rng.choice(list("ACGT"), n))
    # 63, 64, 65 and 129 one-position windows on one template: a wave, a wave and a lane, more than two waves
    t = letters(140)
    alns = [K.aln(t, 0), K.aln(t[:70] + "-" + t[70:], 0, t[:70] + "T" + t[70:]), K.aln(t[3:], 3, t[3:30] + "-" + t[31:]), K.aln(t[:100], 0)]
    for n in (63, 64, 65, 129):
        got, _ = check(ctx, alns, [(p, p + 1, 3) for p in range(n)])
        assert len(got) == n and sum(len(g) for g in got) >= n
    # workspace bounds of the small slot's capacity - 1, the capacity and + 1: the first two run in cns_poa_small, the third in cns_poa_large
    cap = M.cns_poa_small_words()
    parts = [window_of_words(cap + d, 100 * i) for i, d in enumerate((-1, 0, 1))]
    alns = [a for p in parts for a in p[0]]
    assert len(alns) <= 100
    got, info = check(ctx, alns, [p[1] for p in parts])
    assert words_of(info) == [cap - 1, cap, cap + 1] and last_launch() == (1, 1) and all(len(g) > 2 for g in got)
    for p, d in zip(parts, (-1, 0, 1)):
        check(ctx, p[0], [p[1]])
        assert last_launch() == ((1, 1) if d > 0 else (0, 0))
    # 100 pieces on one window; a window of 300 positions no piece covers
    got, info = check(ctx, [K.aln(t[:20], 5)] * 50 + [K.aln(t[:8] + "--" + t[8:20], 5, t[:8] + "GT" + t[8:20])] * 50, [(6, 12, 40), (400, 700, 0), (700, 1000, 5)])
    assert len(got[0]) >= 2 and got[1] == b"N" * 301 and got[2] == b""          # (no piece: every vertex has weight 1; cov 5 asks for 2)
    # six windows of 100 pieces each are large; a budget of 64 KiB makes cns_poa_large run in at least 3 chunks
    alns = [K.aln(t[:90], 0, t[:90])] * 40 + [K.aln(t[:45] + "-" + t[45:90], 0, t[:45] + "A" + t[45:90])] * 60
    windows = [(10 * i + 1, 10 * i + 9, 40) for i in range(6)]
    whole, info = check(ctx, alns, windows)
    assert last_launch() == (6, 1) and min(words_of(info)) > cap
    monkeypatch.setenv("MECAT_CNS_POA_CHUNK_BYTES", str(64 << 10))
    assert hook(ctx, alns, windows) == whole
    assert last_launch()[0] == 6 and last_launch()[1] >= 3


def test_hook_random(ctx):
    """250 seeded templates of up to 2 000 positions and up to 40 alignments (the sizes of test_gpu_cns_pieces.py::test_hook_random)"""
    rng = np.random.default_rng(20266)
    nwin = nbytes = 0
    for _ in range(250):
        L = int(rng.choice([40, 150, 700, 2000]))
        alns, windows = K.random_case(rng, L, int(rng.choice([3, 12, 40])), int(rng.choice([30, 150, 600])) if L > 40 else 30)
        got, _ = check(ctx, alns, P.with_cov(rng, windows, len(alns)))
        nwin += len(got)
        nbytes += sum(len(g) for g in got)
    assert nwin > 5000 and nbytes > 2 * nwin


# ---- the pipeline on the golden accept sets ------------------------------------------------------------------------------------------
FULL = {"pacbio": 240, "nanopore": 160}
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


def run(ctx, g, want, entry="poa", tb=None, ratio=None, params=None):
    import mecat_amd.hip as M
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], 0)
    try:
        f = {"poa": M.cns_accept_templates_poa, "pieces": M.cns_accept_templates_pieces, "plan": M.cns_accept_templates_plan, "ex": M.cns_accept_templates_ex}[entry]
        args = () if entry == "ex" else (params or PR.DEFAULTS[g["tech"]])
        out = f(ctx, vol, g["cands"].copy(), g["tb"] if tb is None else tb, g["tech"], g["mas"], g["ratio"] if ratio is None else ratio, want, *args, threads=16)
        cp = lambda x: np.array(x, copy=True) if isinstance(x, np.ndarray) else ({k: np.array(v, copy=True) for k, v in x.items()} if isinstance(x, dict) else x)
        return tuple(cp(x) for x in out)
    finally:
        vol.free()


def same_outputs(x, y, keys):
    assert x[2] == y[2] and all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x[:2] + x[3:6], y[:2] + y[3:6]))
    assert PR.same_plan(x[6], y[6]) is None
    for k in keys:
        assert x[6][k].tobytes() == y[6][k].tobytes(), k


@pytest.mark.parametrize("name", sorted(FULL))
def test_pipeline(ctx, name):
    import mecat_amd.hip as M
    S, TB, PL, PC, PO = M.CNS_WANT_STRINGS, M.CNS_WANT_TABLE, M.CNS_WANT_PLAN, M.CNS_WANT_PIECES, M.CNS_WANT_POA
    g = golden_set(name, FULL[name])
    full = run(ctx, g, S | PL | PC | PO)
    acc, strings, plan = full[0], full[1], full[6]
    win = plan["windows"]
    assert len(win) > 1000 and len(plan["cns_begin"]) == len(win) + 1 and plan["cns_begin"][0] == 0 and plan["cns_begin"][-1] == len(plan["cns"])
    # the host routine on the call's own strings and pieces: one call over the whole batch (a piece's aln indexes the accepted records)
    windows = np.stack([win["sb"], win["se"], win["cov"]], axis=1).astype(np.int32)
    want, wb, _ = P.host_run_packed(np.ascontiguousarray(strings), acc["str_offset"].astype(np.int64), acc["aln_size"].astype(np.int32), windows, plan["pieces"],
                                    plan["piece_begin"])
    assert np.array_equal(plan["cns_begin"], wb) and plan["cns"].tobytes() == want.tobytes()
    n = np.diff(wb)
    assert (n > 2).mean() > 0.5 and n.max() < 2000          # most windows give something to append
    # PLAN | POA alone: the same bytes, and no strings, tables or pieces
    a, s, nj, tab, idn, begin, p = run(ctx, g, PL | PO)
    assert len(s) == 0 and len(tab) == 0 and len(idn) == 0 and len(begin) == 0 and np.all(a["str_offset"] == -1) and "pieces" not in p
    assert p["cns"].tobytes() == plan["cns"].tobytes() and np.array_equal(p["cns_begin"], plan["cns_begin"]) and PR.same_plan(p, plan) is None
    # everything _pieces returns is what _pieces returns without the bit; without the bit the call is _pieces
    for w in (S | PL | PC, PL | PC, S | TB | PL):
        ref = run(ctx, g, w, entry="pieces")
        keys = ("pieces", "piece_begin") if w & PC else ()
        x = run(ctx, g, w)
        assert "cns" not in x[6]
        same_outputs(x, ref, keys)
        y = run(ctx, g, w | PO)
        same_outputs(y, ref, keys)
        assert y[6]["cns"].tobytes() == plan["cns"].tobytes()


def test_slices_and_templates_without_work(ctx, monkeypatch):
    import mecat_amd.hip as M
    g = golden_set("pacbio", 48)
    params = (4, 3000)
    want = M.CNS_WANT_PLAN | M.CNS_WANT_POA
    one = run(ctx, g, want, params=params)[6]
    assert len(one["windows"]) > 1000 and len(one["cns"]) > 2 * len(one["windows"])
    monkeypatch.setenv("MECAT_CNS_SLICE_JOBS", "1500")          # >= 3 slices: both scratch sets are used again, the slices' strings are put together
    for w in (want, want | M.CNS_WANT_STRINGS | M.CNS_WANT_TABLE | M.CNS_WANT_PIECES):
        many = run(ctx, g, w, params=params)
        assert many[2] > 2 * 1500 and PR.same_plan(one, many[6]) is None
        assert many[6]["cns"].tobytes() == one["cns"].tobytes() and np.array_equal(many[6]["cns_begin"], one["cns_begin"])
    # a template without candidates in the middle of the batch, in slices and in one piece
    tb = np.concatenate([g["tb"][:21], g["tb"][20:]])
    for sliced in (True, False):
        if not sliced:
            monkeypatch.delenv("MECAT_CNS_SLICE_JOBS")
        p = run(ctx, g, want, tb=tb, params=params)[6]
        assert p["windows"].tobytes() == one["windows"].tobytes()
        assert p["cns"].tobytes() == one["cns"].tobytes() and np.array_equal(p["cns_begin"], one["cns_begin"])
    # nothing accepted: no window, no string
    acc, _, nj, _, _, _, p = run(ctx, golden_set("pacbio", 4), want, ratio=1.52)
    assert len(acc) == 0 and nj > 0 and len(p["windows"]) == 0 and len(p["cns"]) == 0 and p["cns_begin"].tolist() == [0]


def test_slice_kinds_at_the_hand_over(ctx, monkeypatch):
    """every template a slice of its own: slices with windows, slices with a table and no window, and a template without candidates
    between them, put together at the hand-over — byte for byte what the batch gives in one slice"""
    import mecat_amd.hip as M
    S, TB, PL, PC, PO = M.CNS_WANT_STRINGS, M.CNS_WANT_TABLE, M.CNS_WANT_PLAN, M.CNS_WANT_PIECES, M.CNS_WANT_POA
    g = golden_set("pacbio", 12)
    tb = np.concatenate([g["tb"][:7], g["tb"][6:]])          # template 6 has no candidates
    kw = dict(tb=tb, ratio=1.0, params=(4, 3000))            # the mapping ratio leaves some templates too few alignments for a segment
    wants = (PL | PO, PL | PC, S | TB | PL | PC | PO)
    one = {w: run(ctx, g, w, **kw) for w in wants}
    p, begin = one[wants[2]][6], one[wants[2]][5]
    seg, sb = p["segments"], p["seg_begin"]
    nwin = np.array([int((seg["win_end"][sb[t]: sb[t + 1]] - seg["win_begin"][sb[t]: sb[t + 1]]).sum()) for t in range(len(tb) - 1)])
    has_table = np.diff(begin) > 0
    assert int((has_table & (nwin == 0)).sum()) >= 1 and int((nwin > 0).sum()) >= 2 and not has_table[6] and nwin.sum() == len(p["windows"])
    monkeypatch.setenv("MECAT_CNS_SLICE_JOBS", "1")
    for w in wants:
        x, y = one[w], run(ctx, g, w, **kw)
        assert x[2] == y[2] and all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(x[:2] + x[3:6], y[:2] + y[3:6]))
        assert sorted(x[6]) == sorted(y[6]) and ("pieces" in x[6]) == bool(w & PC) and ("cns" in x[6]) == bool(w & PO)
        for k in x[6]:
            assert x[6][k].tobytes() == y[6][k].tobytes(), (w, k)
    assert len(one[wants[2]][1]) > 0 and len(p["pieces"]) > 0 and len(p["cns"]) > 0


def test_refusals(ctx):
    import mecat_amd.hip as M
    S, TB, PL, PC, PO = M.CNS_WANT_STRINGS, M.CNS_WANT_TABLE, M.CNS_WANT_PLAN, M.CNS_WANT_PIECES, M.CNS_WANT_POA
    g = golden_set("pacbio", 4)
    for want in (PO, PO | S, PO | TB, PO | PC, PO | PC | S, 0, 32, PL | PO | 32, -1):          # POA without PLAN; unknown bits
        with pytest.raises(M.MhipError, match="want"):
            run(ctx, g, want)
    for entry, want in (("pieces", PL | PO), ("pieces", PL | PC | PO), ("plan", PL | PO), ("ex", S | PO)):      # the older entry points keep refusing the bit
        with pytest.raises(M.MhipError, match="want"):
            run(ctx, g, want, entry=entry)
    # cov < 0 in the hook, and what the piece hook refuses
    with pytest.raises(M.MhipError, match="cov"):
        hook(ctx, [K.FIVE], [(10, 12, -1)])
    for alns, windows, match in (([K.FIVE], [(2, 2, 1)], "sb < se"), ([K.FIVE], [(5, 8, 1), (1, 3, 1)], "ascending"), ([(b"", b"", 3, 3)], [(1, 2, 1)], "len"),
                                 ([K.FIVE] * 101, [(10, 12, 1)], "100")):
        with pytest.raises(M.MhipError, match=match):
            hook(ctx, alns, windows)
    assert hook(ctx, [K.FIVE], []) == [] and hook(ctx, [], [(1, 3, 0), (5, 6, 5)]) == [b"NNN", b""]
