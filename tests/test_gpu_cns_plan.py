"""mecat2cns' consensus plan on the device (mecat_amd/csrc/cns_plan.hip, cns_ranges.h; mhip_cns_accept_templates_plan,
mhip_debug_cns_plan): effective ranges (get_effective_ranges, mecat_correction.cpp:118-153), segments (consensus_worker, :203-239) and the
windows that go to the POA (meap_consensus_one_segment, :81-108).

How it is pinned.  No compiled-reference harness exposes consensus_worker's decisions, so — as the table first was — through
reference-recorded INPUTS (the tables and ident bytes of tests/golden/cns_table.npz, which the unmodified reference produced, and the
accepted coordinates of cns_accept.npz), the loop-by-loop restatement tests/cns_plan_ref.py (held against hand-computed plans in
test_cns_plan_ref_cpu.py) and hand-computed cases here.  Everything goes through the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest

import cns_plan_ref as P
import cns_table_golden as TG
import cns_table_ref as R
import helpers as H

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(H.GOLDEN, "cns_accept.npz"))
F, D, I, U = P.FMAT, P.FDEL, P.FINS, P.UNDS


@pytest.fixture(scope="module")
def ctx():
    import mecat_amd.hip as M
    c = M.Context(0)
    yield c
    c.close()


def tmpl(cov, ident, mranges=()):
    """(table, ident, mapping ranges) of one template: mat_cnt + ins_cnt = cov at every position, split between the two counts"""
    cov = np.asarray(cov, dtype=np.int64)
    t = np.zeros(len(cov), R.TABLE_DTYPE)
    t["base"] = ord("A")
    t["ins_cnt"] = cov // 2
    t["mat_cnt"] = cov - cov // 2
    ident = np.full(len(cov), ident, np.uint8) if np.isscalar(ident) else np.asarray(ident, dtype=np.uint8)
    assert len(ident) == len(cov)
    return t, ident, np.asarray(mranges, dtype=np.int32).reshape(-1, 2)


def hook(ctx, templates, tech, min_cov, min_size):
    import mecat_amd.hip as M
    tb = np.concatenate([[0], np.cumsum([len(t[0]) for t in templates])]).astype(np.int64)
    rb = np.concatenate([[0], np.cumsum([len(t[2]) for t in templates])]).astype(np.int64)
    table = np.concatenate([t[0] for t in templates]) if templates else np.zeros(0, R.TABLE_DTYPE)
    ident = np.concatenate([t[1] for t in templates]) if templates else np.zeros(0, np.uint8)
    ranges = np.concatenate([np.asarray(t[2], np.int32).reshape(-1, 2) for t in templates]) if templates else np.zeros((0, 2), np.int32)
    return M.debug_cns_plan(ctx, table, ident, tb, ranges, rb, tech, min_cov, min_size)


def check(ctx, templates, tech, min_cov, min_size):
    got = hook(ctx, templates, tech, min_cov, min_size)
    want = P.plan(templates, tech, min_cov, min_size)
    assert P.same_plan(got, want) is None, P.same_plan(got, want)
    return got


def well_formed(p, ntmpl):
    """the order and the numbering of a plan, without any restatement"""
    s, w = p["segments"], p["windows"]
    assert len(p["seg_begin"]) == ntmpl + 1 and p["seg_begin"][0] == 0 and p["seg_begin"][-1] == len(s) and np.all(np.diff(p["seg_begin"]) >= 0)
    assert np.array_equal(np.repeat(np.arange(ntmpl), np.diff(p["seg_begin"])), s["template_index"])
    same = s["template_index"][1:] == s["template_index"][:-1]
    assert np.all(s["end"] > s["beg"]) and np.all(s["beg"][1:][same] >= s["end"][:-1][same])
    assert np.array_equal(s["win_begin"], np.concatenate([[0], s["win_end"][:-1]])) and (len(s) == 0 or s["win_end"][-1] == len(w))
    assert np.array_equal(np.repeat(np.arange(len(s)), s["win_end"] - s["win_begin"]), w["segment"])
    ws = s[w["segment"]]
    assert np.all(w["sb"] >= ws["beg"]) and np.all(w["se"] <= ws["end"]) and np.all(w["se"] > w["sb"])
    samew = w["segment"][1:] == w["segment"][:-1]
    assert np.all(w["sb"][1:][samew] >= w["se"][:-1][samew])
    assert len(p["erange_begin"]) == ntmpl + 1 and p["erange_begin"][-1] == len(p["eranges"])


def ids(n, **at):
    """n ident bytes, FINS (neither anchor nor dirty) except where named: ids(9, a=(3, F), b=(5, U))"""
    x = np.full(n, I, np.uint8)
    for pos, v in at.values():
        x[pos] = v
    return x


def test_step_edges(ctx):
    T = []
    for n in (1, 63, 64, 65, 128, 129, 200):
        T.append(tmpl([5] * n, F))                                               # all covered, every position an anchor: no window
        T.append(tmpl([5] * n, F | D))                                           # every anchor dirty: a window per position
        T.append(tmpl([5] * n, U))                                               # no anchor at all
        T.append(tmpl([5] * n, ids(n, a=(n - 1, F), b=(0, U))))                  # dirty in front of the only anchor, which is the last position
        T.append(tmpl([5] * n, ids(n, a=(0, F), b=(n - 1, U))))                  # one window over the whole template, dirty at its last position
    shapes = len(T)
    for e in (63, 64, 65):                                                       # runs ending at positions 63, 64 and 65
        T.append(tmpl([0] * 10 + [5] * (e - 10) + [0] * (200 - e), F | D))
        T.append(tmpl([5] * e + [0] * (129 - e), F))
    T.append(tmpl([0] * 5 + [5] * 185 + [0] * 10, U))                            # a run over three steps
    T.append(tmpl([5] * 200, ids(200, a=(0, F), b=(63, F), c=(30, U), d=(64, D))))      # anchors at lanes 0 and 63
    T.append(tmpl([5] * 200, ids(200, a=(10, F), b=(180, F), c=(100, U))))       # a window over three steps, dirty in the middle step only
    T.append(tmpl([5] * 200, ids(200, a=(10, F), b=(180, F))))                   # ... and the same window clean
    T.append(tmpl([5] * 200, ids(200, a=(10, F | D), b=(180, F))))               # a window dirty only at its anchor, two steps long
    T.append(tmpl([5] * 128, ids(128, a=(100, F), b=(110, D))))                  # the last window ends with the segment on a step boundary
    T.append(tmpl([5] * 128 + [0] * 72, ids(200, a=(100, F), b=(110, D), c=(130, F))))
    T.append(tmpl([5] * 64, ids(64, a=(63, F | U))))                             # an anchor at lane 63 that is the segment's last position
    T.append(tmpl([5] * 200, ids(200, a=(150, F), b=(3, U), c=(70, D), d=(149, U))))     # dirty positions only in front of the first anchor
    got = check(ctx, T, 1, 5, 2)
    well_formed(got, len(T))
    s, w = got["segments"], got["windows"]
    seg_of = lambda t: s[got["seg_begin"][t]: got["seg_begin"][t + 1]]
    win_of = lambda sg: w[sg["win_begin"]: sg["win_end"]]
    # by hand, independent of the restatement
    assert len(seg_of(0)) == 0 and len(seg_of(1)) == 0                           # one position: 1 < 0.95 * 2
    for k, n in enumerate((63, 64, 65, 128, 129, 200), start=1):
        a, b, c, d, e = (seg_of(5 * k + j) for j in range(5))
        assert [x.tolist() for x in (a[["beg", "end", "n_anchors"]], b[["beg", "end", "n_anchors"]], c[["beg", "end", "n_anchors"]])] == [[(0, n, n)], [(0, n, n)], [(0, n, 0)]]
        assert len(win_of(a[0])) == 0 and len(win_of(c[0])) == 0 and len(win_of(d[0])) == 0
        assert np.array_equal(win_of(b[0])["sb"], np.arange(n)) and np.array_equal(win_of(b[0])["se"], np.arange(1, n + 1))
        assert win_of(e[0]).tolist() == [(0, n, 5, got["seg_begin"][5 * k + 4])]
    t = shapes
    for e in (63, 64, 65):
        assert seg_of(t)[["beg", "end"]].tolist() == [(10, e)] and seg_of(t + 1)[["beg", "end"]].tolist() == [(0, e)]
        t += 2
    assert seg_of(t)[["beg", "end", "n_anchors"]].tolist() == [(5, 190, 0)]
    assert win_of(seg_of(t + 1)[0])[["sb", "se"]].tolist() == [(0, 63), (63, 200)]
    assert win_of(seg_of(t + 2)[0])[["sb", "se", "cov"]].tolist() == [(10, 180, 5)]
    assert len(win_of(seg_of(t + 3)[0])) == 0
    assert win_of(seg_of(t + 4)[0])[["sb", "se"]].tolist() == [(10, 180)]
    assert win_of(seg_of(t + 5)[0])[["sb", "se"]].tolist() == [(100, 128)]
    assert seg_of(t + 6)[["beg", "end"]].tolist() == [(0, 128)] and win_of(seg_of(t + 6)[0])[["sb", "se"]].tolist() == [(100, 128)]
    assert win_of(seg_of(t + 7)[0])[["sb", "se"]].tolist() == [(63, 64)]
    assert seg_of(t + 8)["n_anchors"].tolist() == [1] and len(win_of(seg_of(t + 8)[0])) == 0


def min_run(min_size):
    n = int(0.95 * min_size)
    while float(n) < 0.95 * min_size:
        n += 1
    return n


def test_thresholds(ctx):
    for min_size in range(2, 201):
        thr = min_run(min_size)
        assert float(thr) >= 0.95 * min_size > float(thr - 1)
        # runs of thr - 1, thr, thr + 1 positions at exactly min_cov, one position of min_cov - 1 between them
        cov = [0] * 3 + [7] * (thr - 1) + [6] + [7] * thr + [6] + [7] * (thr + 1) + [6] * 2
        got = check(ctx, [tmpl(cov, F | U)], 1, 7, min_size)
        b1 = 3 + thr - 1 + 1
        b2 = b1 + thr + 1
        assert got["segments"][["beg", "end"]].tolist() == [(b1, b1 + thr), (b2, b2 + thr + 1)], min_size
        assert len(got["windows"]) == 2 * thr + 1 and np.all(got["windows"]["cov"] == 7)
    # the counts are unsigned bytes, their sum an int: 100 + 100
    t = np.zeros(10, R.TABLE_DTYPE)
    t["mat_cnt"][2:8] = 100
    t["ins_cnt"][2:8] = 100
    t["mat_cnt"][8] = 199
    one = (t, np.full(10, F | D, np.uint8), np.zeros((0, 2), np.int32))
    got = check(ctx, [one], 1, 200, 4)
    assert got["segments"][["beg", "end"]].tolist() == [(2, 8)] and np.all(got["windows"]["cov"] == 200) and len(got["windows"]) == 6
    assert len(check(ctx, [one], 1, 201, 4)["segments"]) == 0
    assert check(ctx, [one], 1, 199, 4)["segments"][["beg", "end"]].tolist() == [(2, 9)]


def test_ranges_cut_runs(ctx):
    L = 4000
    cov = [9] * L
    ident = np.full(L, I, np.uint8)
    ident[::37] = F
    ident[5::101] = U
    touching = [(600, 2000), (2000, 3400)]           # overlap 0 < 1000: effective ranges (600, 2000) and (2000, 3400); no alignment spans the read
    got = check(ctx, [tmpl(cov, ident, touching)], 0, 4, 1000)
    assert got["eranges"].tolist() == [[600, 2000], [2000, 3400]] and got["segments"][["beg", "end"]].tolist() == [(600, 2000), (2000, 3400)]
    # 0.95 * 1500 = 1425 > 1400: neither piece is long enough — although the covered run, and the two ranges together, are
    got = check(ctx, [tmpl(cov, ident, touching)], 0, 4, 1500)
    assert len(got["eranges"]) == 0 and len(got["segments"]) == 0
    # one range that ends in the middle of the covered run; the run ends with it
    got = check(ctx, [tmpl(cov, ident, [(600, 2000)])], 0, 4, 1000)
    assert got["segments"][["beg", "end"]].tolist() == [(600, 2000)]
    # an alignment over (nearly) the whole read: one range (0, L) whatever min_size; nothing accepted: nothing
    got = check(ctx, [tmpl(cov, ident, [(500, 3500)]), tmpl(cov, ident)], 0, 4, 4000)
    assert got["eranges"].tolist() == [[0, L]] and got["segments"][["template_index", "beg", "end"]].tolist() == [(0, 0, L)]
    # tech 1 without mapping ranges: the whole read
    got = check(ctx, [tmpl(cov, ident), tmpl([9] * 70 + [0] * 30, F | D)], 1, 4, 50)
    assert got["eranges"].tolist() == [[0, L], [0, 100]] and got["segments"][["template_index", "beg", "end"]].tolist() == [(0, 0, L), (1, 0, 70)]


def test_range_function(ctx):
    """300 random sets of up to 100 mapping ranges on reads of 2 000 to 40 000 bases, equal starts and equal pairs among them: the
    effective ranges the library computes (host code, in the accept replay and in the hook) are the restatement's"""
    rng = np.random.default_rng(41)
    kept = whole = 0
    for call, min_size in enumerate((5000, 2000, 300)):
        T, want = [], []
        for _ in range(100):
            L = int(rng.integers(2000, 40001))
            n = int(rng.integers(0, 101))
            lo = int(rng.choice([0, 400, 501, 600, 1500]))
            start = rng.integers(lo, L - 1, n)
            length = rng.integers(1, max(2, L // int(rng.choice([2, 4, 10]))), n)
            end = np.minimum(start + length, L - int(rng.choice([0, 400, 501, 600])))
            end = np.maximum(end, start)
            m = np.stack([start, end], axis=1).astype(np.int32)
            if n >= 4:
                m[1, 0] = m[0, 0]                                   # equal starts
                m[1, 1] = max(m[1, 1], m[1, 0])
                m[3] = m[2]                                         # an equal pair
            if n and rng.random() < 0.4:                            # one alignment over the whole read, or just short of it at either end
                m[n // 2] = (int(rng.choice([0, 500, 501])), L - int(rng.choice([0, 500, 501])))
            assert np.all(m[:, 0] <= m[:, 1]) and np.all(m[:, 1] <= L) and np.all(m[:, 0] >= 0)
            T.append((np.zeros(L, R.TABLE_DTYPE), np.zeros(L, np.uint8), m))
            want.append(P.effective_ranges(m.tolist(), L, 0, min_size))
        got = hook(ctx, T, 0, 4, min_size)
        assert np.array_equal(got["erange_begin"], np.concatenate([[0], np.cumsum([len(w) for w in want])]))
        assert got["eranges"].tolist() == [list(r) for w in want for r in w]
        assert len(got["segments"]) == 0 and len(got["windows"]) == 0
        kept += sum(len(w) for w in want)
        whole += sum(1 for w, t in zip(want, T) if w == [(0, len(t[0]))])
    assert kept > 300 and 10 <= whole <= 290, (kept, whole)          # the sweep and the whole-read shortcut are both exercised


def test_random_tables(ctx):
    rng = np.random.default_rng(42)
    T = []
    for k in range(200):
        n = int(rng.integers(0, 301)) if k % 20 else 0                     # (every twentieth template is empty)
        cov = np.repeat(rng.choice([0, 3, 4, 9, 200], 40), rng.integers(1, 40, 40))[:n]
        cov = np.concatenate([cov, np.zeros(n - len(cov), np.int64)])
        ident = np.where(rng.random(n) < rng.choice([0.02, 0.2, 0.8]), F, 0) | np.where(rng.random(n) < 0.1, U, 0) | np.where(rng.random(n) < 0.1, D, 0) | \
            np.where(rng.random(n) < 0.2, I, 0)
        T.append(tmpl(cov, ident.astype(np.uint8), [(0, n)] if n and k % 7 else []))
    got = check(ctx, T, 0, 4, 10)
    well_formed(got, len(T))
    assert len(got["segments"]) > 100 and len(got["windows"]) > 300 and (np.diff(got["seg_begin"]) > 1).any() and (np.diff(got["seg_begin"]) == 0).any()
    got1 = check(ctx, T, 1, 4, 10)
    assert len(got1["segments"]) > len(got["segments"])                   # tech 1 plans the templates without mapping ranges too
    assert P.same_plan(got, hook(ctx, T, 0, 4, 10)) is None               # the same bytes on every run


# ---- the pipeline on the golden accept sets ------------------------------------------------------------------------------------------
FULL = {"pacbio": 240, "nanopore": 160}
_sets, _runs = {}, {}


def golden_set(name, K):
    if (name, K) not in _sets:
        from mecat_amd import workload as W
        n, L, Gn, seed, ont, tech, mas = (int(x) for x in G[name + "_par"])
        err, ratio = (float(x) for x in G[name + "_ratio"])
        codes, lens = W.synth_reads(n, L, err, Gn, seed, ont)
        pac, offs, nb = W.pack_volume(codes, lens)
        tb = G[name + "_tmpl_begin"][: K + 1].copy()
        _sets[name, K] = dict(pac=pac, offs=offs, nb=nb, lens=lens, K=K, tb=tb, cands=G[name + "_cands"][: tb[K]].copy(), tech=tech, mas=mas, ratio=ratio)
    return _sets[name, K]


def run_plan(ctx, g, want, plan=True, tb=None, ratio=None, params=None):
    """mhip_cns_accept_templates_plan (plan=False: mhip_cns_accept_templates_ex) -> its tuple, arrays copied"""
    import mecat_amd.hip as M
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], 0)
    try:
        tb = g["tb"] if tb is None else tb
        ratio = g["ratio"] if ratio is None else ratio
        if plan:
            out = M.cns_accept_templates_plan(ctx, vol, g["cands"].copy(), tb, g["tech"], g["mas"], ratio, want, *(params or P.DEFAULTS[g["tech"]]), threads=16)
        else:
            out = M.cns_accept_templates_ex(ctx, vol, g["cands"].copy(), tb, g["tech"], g["mas"], ratio, want, threads=16)
        return tuple(np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in out)
    finally:
        vol.free()


def full_run(ctx, name, want, plan=True):
    """the whole golden set at the defaults, run once per mode and shared (read-only)"""
    if (name, want, plan) not in _runs:
        _runs[name, want, plan] = run_plan(ctx, golden_set(name, FULL[name]), want, plan)
    return _runs[name, want, plan]


def recorded8(name):
    """the first 8 templates of a set as the unmodified reference left them: (table, ident, golden (soff, send))"""
    T = TG.golden()
    table, ident, b8 = TG.planes_to_table(T[name + "_table8"]), T[name + "_ident8"], T[name + "_begin8"]
    first = np.concatenate([[0], np.cumsum(G[name + "_nacc"])])
    return [(table[b8[t]: b8[t + 1]], ident[b8[t]: b8[t + 1]], G[name + "_meta"][first[t]: first[t + 1], :2]) for t in range(8)]


def head_of(p, k):
    """the plan of the first k templates of a plan (segments and windows come in template order: a prefix)"""
    ns, ne = int(p["seg_begin"][k]), int(p["erange_begin"][k])
    nw = int(p["segments"]["win_end"][ns - 1]) if ns else 0
    return dict(segments=p["segments"][:ns], seg_begin=p["seg_begin"][: k + 1], windows=p["windows"][:nw], eranges=p["eranges"][:ne], erange_begin=p["erange_begin"][: k + 1])


@pytest.mark.parametrize("name", sorted(FULL))
def test_pipeline_plan_on_the_golden_set(ctx, name):
    import mecat_amd.hip as M
    n = FULL[name]
    g = golden_set(name, n)
    tech = g["tech"]
    S, TB, PL = M.CNS_WANT_STRINGS, M.CNS_WANT_TABLE, M.CNS_WANT_PLAN
    a_p, s_p, nj_p, t_p, i_p, b_p, plan = full_run(ctx, name, PL)
    a_tp, s_tp, nj_tp, t_tp, i_tp, b_tp, plan_tp = full_run(ctx, name, TB | PL)
    a_stp, s_stp, nj_stp, t_stp, i_stp, b_stp, plan_stp = full_run(ctx, name, S | TB | PL)
    # 1. the three modes give the same plan; with PLAN alone nothing else comes back
    assert P.same_plan(plan, plan_tp) is None and P.same_plan(plan, plan_stp) is None
    well_formed(plan, n)
    assert len(s_p) == 0 and len(t_p) == 0 and len(i_p) == 0 and len(b_p) == 0 and np.all(a_p["str_offset"] == -1) and len(s_tp) == 0
    # 2. everything else is what mhip_cns_accept_templates_ex returns for the same `want` without PLAN
    a_t, s_t, nj_t, t_t, i_t, b_t = full_run(ctx, name, TB, plan=False)
    a_st, s_st, nj_st, t_st, i_st, b_st = full_run(ctx, name, S | TB, plan=False)
    assert np.array_equal(a_tp, a_t) and t_tp.tobytes() == t_t.tobytes() and i_tp.tobytes() == i_t.tobytes() and np.array_equal(b_tp, b_t) and nj_tp == nj_t
    assert np.array_equal(a_stp, a_st) and s_stp.tobytes() == s_st.tobytes() and t_stp.tobytes() == t_st.tobytes() and i_stp.tobytes() == i_st.tobytes()
    assert np.array_equal(b_stp, b_st) and nj_stp == nj_st == nj_p and np.array_equal(a_p, a_t) and len(s_st) > 0
    # 3. the first 8 templates: the restatement on the table, the ident bytes and the coordinates the unmodified reference recorded
    want8 = P.plan(recorded8(name), tech, *P.DEFAULTS[tech])
    assert P.same_plan(head_of(plan, 8), want8) is None, P.same_plan(head_of(plan, 8), want8)
    # 4. all templates: the hook on the pipeline's own table, with the accepted coordinates as mapping ranges
    first = np.concatenate([[0], np.cumsum(np.bincount(a_tp["template_index"], minlength=n))])
    m = np.stack([a_tp["soff"], a_tp["send"]], axis=1).astype(np.int32)
    import mecat_amd.hip as M
    hooked = M.debug_cns_plan(ctx, t_tp, i_tp, b_tp, m, first, tech, *P.DEFAULTS[tech])
    assert P.same_plan(plan, hooked) is None, P.same_plan(plan, hooked)


def test_the_golden_sets_test_something(ctx):
    """at least half of the sixteen recorded templates yield a segment, and the sixteen together at least 1 000 windows — on the device"""
    import mecat_amd.hip as M
    with_seg = nwin = 0
    for name in sorted(FULL):
        p = head_of(full_run(ctx, name, M.CNS_WANT_PLAN)[6], 8)
        with_seg += int((np.diff(p["seg_begin"]) > 0).sum())
        nwin += len(p["windows"])
    assert with_seg >= 8 and nwin >= 1000, (with_seg, nwin)


def test_slices_and_templates_without_work(ctx, monkeypatch):
    import mecat_amd.hip as M
    g = golden_set("pacbio", 48)
    params = (4, 3000)          # (more segments than at 5000: a shorter run is enough)
    want = M.CNS_WANT_TABLE | M.CNS_WANT_PLAN
    one = run_plan(ctx, g, want, params=params)
    assert one[2] > 2 * 1500 and len(one[6]["segments"]) >= 12 and len(one[6]["windows"]) > 1000
    monkeypatch.setenv("MECAT_CNS_SLICE_JOBS", "1500")          # >= 3 slices: both scratch sets are used again, the pieces are put together
    for w in (want, M.CNS_WANT_PLAN):
        many = run_plan(ctx, g, w, params=params)
        assert P.same_plan(one[6], many[6]) is None, P.same_plan(one[6], many[6])
        assert np.array_equal(many[0]["soff"], one[0]["soff"]) and (w == M.CNS_WANT_PLAN or many[3].tobytes() == one[3].tobytes())
    # a template without candidates in the middle of the batch, in slices and in one piece
    tb = np.concatenate([g["tb"][:21], g["tb"][20:]])
    for sliced in (True, False):
        if not sliced:
            monkeypatch.delenv("MECAT_CNS_SLICE_JOBS")
        p = run_plan(ctx, g, M.CNS_WANT_PLAN, tb=tb, params=params)[6]
        well_formed(p, 49)
        assert p["seg_begin"][20] == p["seg_begin"][21] and p["erange_begin"][20] == p["erange_begin"][21]
        assert np.array_equal(np.delete(p["seg_begin"], 21), one[6]["seg_begin"]) and np.array_equal(np.delete(p["erange_begin"], 21), one[6]["erange_begin"])
        assert np.array_equal(p["segments"]["template_index"], one[6]["segments"]["template_index"] + (one[6]["segments"]["template_index"] >= 20))
        assert all(np.array_equal(p["segments"][f], one[6]["segments"][f]) for f in ("beg", "end", "n_anchors", "win_begin", "win_end"))
        assert p["windows"].tobytes() == one[6]["windows"].tobytes() and np.array_equal(p["eranges"], one[6]["eranges"])
    # templates with candidates of which none is accepted (no alignment reaches 1.5 times a read's length): PacBio has no range then,
    # nanopore the whole read, and neither has a segment
    for name in sorted(FULL):
        g4 = golden_set(name, 4)
        acc, _, nj, table, ident, begin, p = run_plan(ctx, g4, want, ratio=1.52)
        assert len(acc) == 0 and nj > 0 and np.array_equal(np.diff(begin), g4["lens"][:4]) and np.all(table["mat_cnt"] == 0)
        assert len(p["segments"]) == 0 and len(p["windows"]) == 0 and p["seg_begin"].tolist() == [0] * 5
        assert p["eranges"].tolist() == ([[0, int(x)] for x in g4["lens"][:4]] if g4["tech"] else [])


def test_refusals(ctx):
    import mecat_amd.hip as M
    g = golden_set("pacbio", 4)
    for want, params, match in ((0, (4, 5000), "want"), (8, (4, 5000), "want"), (M.CNS_WANT_PLAN | 8, (4, 5000), "want"), (M.CNS_WANT_PLAN, (4, 1), "min_size"),
                                (M.CNS_WANT_PLAN, (0, 5000), "min_cov"), (M.CNS_WANT_TABLE | M.CNS_WANT_PLAN, (4, -5), "min_size")):
        with pytest.raises(M.MhipError, match=match):
            run_plan(ctx, g, want, params=params)
    with pytest.raises(M.MhipError, match="want"):
        run_plan(ctx, g, M.CNS_WANT_PLAN, plan=False)                            # mhip_cns_accept_templates_ex still refuses bit 4
    with pytest.raises(M.MhipError, match="want"):
        run_plan(ctx, g, M.CNS_WANT_TABLE | M.CNS_WANT_PLAN, plan=False)
    # PLAN without a place to put it: the C entry point itself, NULL for the six plan outputs
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], 0)
    try:
        cands, tb = g["cands"].copy(), np.ascontiguousarray(g["tb"], dtype=np.int64)
        acc, st, tab, idn, tbeg = (C.c_void_p() for _ in range(5))
        na, sb, nj = C.c_int64(), C.c_int64(), C.c_int64()
        rc = M.lib().mhip_cns_accept_templates_plan(ctx.h, vol.h, cands.ctypes.data, tb.ctypes.data, len(tb) - 1, g["tech"], g["mas"], g["ratio"], 4, M.CNS_WANT_PLAN, 4,
                                                    5000, C.byref(acc), C.byref(na), C.byref(st), C.byref(sb), C.byref(nj), C.byref(tab), C.byref(idn), C.byref(tbeg),
                                                    None, None, None, None, None, None)
        assert rc != 0 and b"plan" in M.lib().mhip_last_error() and not acc.value and not tab.value
    finally:
        vol.free()
    # the hook refuses the same parameters, and a mapping range that leaves its template
    one = tmpl([5] * 10, F)
    for params, match in (((4, 1), "min_size"), ((0, 10), "min_cov")):
        with pytest.raises(M.MhipError, match=match):
            hook(ctx, [one], 1, *params)
    with pytest.raises(M.MhipError, match="leaves"):
        hook(ctx, [tmpl([5] * 10, F, [(2, 11)])], 0, 4, 10)
