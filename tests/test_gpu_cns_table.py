"""mecat2cns' consensus table built on the device in the accept stage (mecat_amd/csrc/cns_table.hip; mhip_cns_accept_templates_ex,
mhip_debug_cns_table): what meap_add_one_aln (mecat_correction.cpp:36-60) folds the accepted strings into, and the ident byte
identify_one_consensus_item (:14-24) gives every position.

How it is pinned.  TO THE COMPILED, UNMODIFIED REFERENCE, as every other device stage of the mecat2cns path:
oracle/_ref/libref_cns_table.so (oracle/ref_harness_cns_table.cpp holds mecat_correction.cpp itself) exposes the table a template is left
with, meap_add_one_aln and identify_one_consensus_item, and tests/golden/cns_table.npz (make_golden_cns_table.py) records what they give:
  * the table and ident bytes of all 240 + 160 templates of the golden accept sets, as a SHA-256 per template and in full for the first 8
    of each set: the pipeline (CNS_WANT_TABLE alone) must give those bytes
  * the ident byte of every count triple a position can hold (mat + ins <= 100, del <= mat + ins): one hook call builds exactly those
    counts on a template of 348 551 letters
  * meap_add_one_aln on 1 060 adversarial pairs (the reference's own normalize_gaps outputs of pushgaps.npz, and generated pairs with long
    template-gap runs: beginning with double gaps, double gaps only, at the first and last column, at soff == 0), guards included
  * a volume whose first read id is not 0 must give the bytes of the same reads numbered from 0.
tests/cns_table_ref.py, the restatement of the rules, is held against the same recorded results on the CPU (test_cns_table_ref_cpu.py)
and stays the checker of the kernels' own corner cases through the test hook (64-column steps, runs across steps, byte carries) and of
the subset test below, which also shows that the strings are the reference's and checks one property without any restatement:
mat_cnt + ins_cnt at a position is the number of accepted alignments covering it, from the golden coordinates alone."""
import hashlib
import os

import numpy as np
import pytest

import cns_table_golden as TG
import cns_table_ref as R
import helpers as H

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(H.GOLDEN, "cns_accept.npz"))
LET = np.frombuffer(b"ACGT", dtype=np.uint8)
MATCH, QGAP, SGAP, BOTH = 0, 1, 2, 3          # column kinds: q == s / '-' over a base / a base over '-' / '-' over '-'


@pytest.fixture(scope="module")
def ctx():
    import mecat_amd.hip as M
    c = M.Context(0)
    yield c
    c.close()


def make_aln(tmpl, soff, ops, rng):
    """(q, s, soff) with the given column kinds over template letters tmpl[soff:]"""
    ops = np.asarray(ops)
    takes = (ops == MATCH) | (ops == QGAP)
    p = soff + np.cumsum(takes) - takes
    assert soff >= 0 and soff + int(takes.sum()) <= len(tmpl)
    s = np.where(takes, tmpl[np.minimum(p, len(tmpl) - 1)], R.GAP).astype(np.uint8)
    q = np.where(ops == MATCH, s, np.where(ops == SGAP, LET[rng.integers(0, 4, len(ops))], R.GAP)).astype(np.uint8)
    return q, s, soff


def lay_out(alns, lead=0):
    """the accept stage's layout: q, NUL, s, NUL, back to back"""
    off, pos = [], lead
    for q, _, _ in alns:
        off.append(pos)
        pos += 2 * (len(q) + 1)
    buf = np.zeros(pos + 8, dtype=np.uint8)
    for o, (q, s, _) in zip(off, alns):
        buf[o: o + len(q)] = q
        buf[o + len(q) + 1: o + 2 * len(q) + 1] = s
    return buf, np.array(off, np.int64), np.array([len(a[0]) for a in alns], np.int32), np.array([a[2] for a in alns], np.int32)


def check_hook(ctx, alns, tmpl, lead=0):
    import mecat_amd.hip as M
    table, ident = M.debug_cns_table(ctx, *lay_out(alns, lead), tmpl.tobytes())
    want_t, want_i = R.build_table(alns, tmpl)
    assert table.tobytes() == want_t.tobytes(), np.nonzero(table.view(np.uint32) != want_t.view(np.uint32))[0][:10]
    assert ident.tobytes() == want_i.tobytes()
    return table, ident


def ops_with(n, **runs):
    ops = np.zeros(n, dtype=np.int64)
    for k, (a, b, kind) in runs.items():
        ops[a:b] = kind
    return ops


def test_hook_single_alignments_and_runs_across_steps(ctx):
    rng = np.random.default_rng(5)
    tmpl = LET[rng.integers(0, 4, 400)]
    for n in (1, 63, 64, 65, 128, 129):
        check_hook(ctx, [make_aln(tmpl, 3, np.zeros(n, np.int64), rng)], tmpl)                                    # all match
        check_hook(ctx, [make_aln(tmpl, 3, rng.choice([0, 0, 0, 0, 1, 2, 2, 3], n), rng)], tmpl, lead=n % 7)     # every kind of column
    shapes = {
        "run from column 63": ops_with(130, r=(63, 66, SGAP)),
        "run from column 64": ops_with(130, r=(64, 66, SGAP)),
        "run over three steps": ops_with(260, r=(60, 201, SGAP)),
        "three steps, bases only in the last": ops_with(260, a=(60, 190, BOTH), b=(190, 201, SGAP)),
        "three steps, a base in the first only": ops_with(260, a=(60, 61, SGAP), b=(61, 201, BOTH)),
        "three steps, bases in each": ops_with(260, a=(60, 201, BOTH), b=(62, 63, SGAP), c=(100, 101, SGAP), d=(130, 131, SGAP)),
        "run ends with its step": ops_with(130, r=(50, 64, SGAP)),
        "run fills one step": ops_with(200, r=(64, 128, SGAP)),
        "double gaps to the step's end, base behind it": ops_with(130, a=(60, 70, BOTH), b=(70, 71, SGAP)),
        "a run of double gaps only": ops_with(100, r=(10, 15, BOTH)),
        "double gaps only, across a step": ops_with(130, r=(60, 70, BOTH)),
        "insertions around a step": ops_with(130, r=(62, 67, QGAP)),
        "run at the end of the strings": ops_with(70, r=(66, 70, SGAP)),
    }
    no_del = ("a run of double gaps only", "double gaps only, across a step", "insertions around a step")
    for name, ops in shapes.items():
        table, _ = check_hook(ctx, [make_aln(tmpl, 5, ops, rng)], tmpl)
        assert int(table["del_cnt"].sum()) == (0 if name in no_del else 1), name          # one run, one deletion — if it holds a base
    # a run in front of the first template base at soff == 0: the reference would count below its array; nothing is written
    table, _ = check_hook(ctx, [make_aln(tmpl, 0, ops_with(80, r=(0, 3, SGAP)), rng)], tmpl)
    assert int(table["del_cnt"].sum()) == 0 and int(table["mat_cnt"].sum()) == 77
    table, _ = check_hook(ctx, [make_aln(tmpl, 0, ops_with(150, r=(0, 70, SGAP)), rng)], tmpl)
    assert int(table["del_cnt"].sum()) == 0
    # the last template position and a deletion behind it
    check_hook(ctx, [make_aln(tmpl, 400 - 66, ops_with(70, r=(66, 70, SGAP)), rng)], tmpl)


def test_hook_255_alignments_do_not_carry_between_bytes(ctx):
    rng = np.random.default_rng(6)
    tmpl = LET[rng.integers(0, 4, 70)]
    one = make_aln(tmpl, 0, np.zeros(70, np.int64), rng)
    table, ident = check_hook(ctx, [one] * 255, tmpl)
    assert np.all(table["mat_cnt"] == 255) and np.all(table["ins_cnt"] == 0) and np.all(table["del_cnt"] == 0)
    assert np.array_equal(table["base"], tmpl) and np.all(ident == R.FMAT)
    # the same for the other two bytes: 255 insertions and 255 deletions per position
    ops = np.zeros(140, np.int64)
    ops[0::2] = QGAP
    ops[1::2] = SGAP
    table, _ = check_hook(ctx, [make_aln(tmpl, 0, ops, rng)] * 255, tmpl)
    assert np.all(table["mat_cnt"] == 0) and np.all(table["ins_cnt"] == 255) and np.all(table["del_cnt"] == 255) and np.all(table["base"] == ord("N"))


def test_hook_100_random_alignments_on_overlapping_spans(ctx):
    rng = np.random.default_rng(7)
    tmpl = LET[rng.integers(0, 4, 1500)]
    alns = []
    for _ in range(100):
        soff = int(rng.integers(0, 300))
        ops = rng.choice([MATCH, QGAP, SGAP, BOTH], int(rng.integers(700, 1200)), p=[0.8, 0.07, 0.1, 0.03])
        keep = np.cumsum((ops == MATCH) | (ops == QGAP)) <= len(tmpl) - soff
        alns.append(make_aln(tmpl, soff, ops[keep], rng))
    table, ident = check_hook(ctx, alns, tmpl, lead=3)
    assert table["mat_cnt"].max() > 60 and table["del_cnt"].max() > 5 and len(set(ident.tolist())) >= 4


def test_hook_refuses_what_it_cannot_tally(ctx):
    import mecat_amd.hip as M
    rng = np.random.default_rng(8)
    tmpl = LET[rng.integers(0, 4, 70)]
    one = make_aln(tmpl, 0, np.zeros(70, np.int64), rng)
    with pytest.raises(M.MhipError, match="255"):
        M.debug_cns_table(ctx, *lay_out([one] * 256), tmpl.tobytes())
    q = one[0].copy()
    q[9] = LET[(int(np.nonzero(LET == q[9])[0][0]) + 1) % 4]
    with pytest.raises(M.MhipError, match="mismatch"):
        M.debug_cns_table(ctx, *lay_out([(q, one[1], 0)]), tmpl.tobytes())
    with pytest.raises(M.MhipError, match="leaves the template"):
        M.debug_cns_table(ctx, *lay_out([(one[0], one[1], 1)]), tmpl.tobytes())
    with pytest.raises(M.MhipError, match="leaves the template"):
        M.debug_cns_table(ctx, *lay_out([(one[0][:5], one[1][:5], -1)]), tmpl.tobytes())


# ---- the pipeline on the reference-pinned golden --------------------------------------------------------------------------------------
SUBSET = {"pacbio": 48, "nanopore": 32}
_volumes = {}


def golden_subset(name, K=None):
    """(ctx-free inputs of the first K templates of a golden set, built once)"""
    K = SUBSET[name] if K is None else K
    if (name, K) not in _volumes:
        from mecat_amd import workload as W
        n, L, Gn, seed, ont, tech, mas = (int(x) for x in G[name + "_par"])
        err, ratio = (float(x) for x in G[name + "_ratio"])
        codes, lens = W.synth_reads(n, L, err, Gn, seed, ont)
        pac, offs, nb = W.pack_volume(codes, lens)
        tb = G[name + "_tmpl_begin"][: K + 1].copy()
        starts = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
        letters = [LET[codes[starts[t]: starts[t + 1]]] for t in range(K)]
        _volumes[name, K] = dict(pac=pac, offs=offs, nb=nb, lens=lens, K=K, tb=tb, cands=G[name + "_cands"][: tb[K]].copy(), tech=tech, mas=mas, ratio=ratio,
                              letters=letters, nacc=G[name + "_nacc"][:K], sha=G[name + "_sha"][:K], meta=G[name + "_meta"][: int(G[name + "_nacc"][:K].sum())])
    return _volumes[name, K]


def run_ex(ctx, g, want, tb=None, cands=None, start_id=0):
    import mecat_amd.hip as M
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], start_id)
    try:
        out = M.cns_accept_templates_ex(ctx, vol, (g["cands"] if cands is None else cands).copy(), g["tb"] if tb is None else tb, g["tech"], g["mas"], g["ratio"],
                                        want, threads=16)
        return tuple(np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in out)
    finally:
        vol.free()


@pytest.fixture(scope="module")
def both(ctx):
    """STRINGS | TABLE on either subset, run once and shared (read-only)"""
    import mecat_amd.hip as M
    return {name: run_ex(ctx, golden_subset(name), M.CNS_WANT_STRINGS | M.CNS_WANT_TABLE) for name in SUBSET}


@pytest.mark.parametrize("name", sorted(SUBSET))
def test_pipeline_table_of_the_reference_strings(both, name):
    g = golden_subset(name)
    acc, strings, njobs, table, ident, begin = both[name]
    K = g["K"]
    assert njobs == int(np.minimum(np.diff(g["tb"]), 200).sum())
    # 1. the accepted alignments and their strings are the unmodified reference's
    assert np.array_equal(np.bincount(acc["template_index"], minlength=K), g["nacc"])
    assert np.array_equal(np.stack([acc["soff"], acc["send"], acc["aln_size"]], axis=1), g["meta"])
    first = np.concatenate([[0], np.cumsum(g["nacc"])])
    for t in range(K):
        a = acc[first[t]: first[t + 1]]
        lo, hi = int(a["str_offset"][0]), int(a["str_offset"][-1]) + 2 * (int(a["aln_size"][-1]) + 1)
        assert hashlib.sha256(strings[lo:hi]).hexdigest() == str(g["sha"][t]), t
    # 2. one table per template, one item per base of the read
    assert np.array_equal(np.diff(begin), g["lens"][:K]) and begin[0] == 0 and len(table) == len(ident) == begin[K]
    for t in range(K):
        a = acc[first[t]: first[t + 1]]
        alns = [(strings[o: o + n], strings[o + n + 1: o + 2 * n + 1], so) for o, n, so in zip(a["str_offset"].tolist(), a["aln_size"].tolist(), a["soff"].tolist())]
        want_t, want_i = R.build_table(alns, g["letters"][t])
        got = table[begin[t]: begin[t + 1]]
        assert got.tobytes() == want_t.tobytes(), (t, np.nonzero(got.view(np.uint32) != want_t.view(np.uint32))[0][:10])
        assert ident[begin[t]: begin[t + 1]].tobytes() == want_i.tobytes(), t
        # 3. without the restatement: every accepted alignment has a match or an insertion column at each position of [soff, send)
        cover = np.zeros(len(got) + 1, dtype=np.int64)
        np.add.at(cover, g["meta"][first[t]: first[t + 1], 0], 1)
        np.add.at(cover, g["meta"][first[t]: first[t + 1], 1], -1)
        assert np.array_equal(got["mat_cnt"].astype(np.int64) + got["ins_cnt"], np.cumsum(cover)[:-1]), t
    assert table["del_cnt"].max() > 0 and table["ins_cnt"].max() > 0 and (ident == 7).any() and (ident & R.UNDS).any()


def test_table_only_and_slices_change_nothing(ctx, both, monkeypatch):
    import mecat_amd.hip as M
    g = golden_subset("pacbio")
    acc, strings, njobs, table, ident, begin = both["pacbio"]
    a2, s2, nj2, t2, i2, b2 = run_ex(ctx, g, M.CNS_WANT_TABLE)
    assert len(s2) == 0 and np.all(a2["str_offset"] == -1) and nj2 == njobs
    names = [f for f in acc.dtype.names if f != "str_offset"]
    assert all(np.array_equal(a2[f], acc[f]) for f in names)
    assert t2.tobytes() == table.tobytes() and i2.tobytes() == ident.tobytes() and np.array_equal(b2, begin)
    assert njobs > 2 * 1500
    monkeypatch.setenv("MECAT_CNS_SLICE_JOBS", "1500")          # more jobs than two slices hold: >= 3 slices, both buffer sets are used again
    for want in (M.CNS_WANT_STRINGS | M.CNS_WANT_TABLE, M.CNS_WANT_TABLE):
        a3, s3, nj3, t3, i3, b3 = run_ex(ctx, g, want)
        if want & M.CNS_WANT_STRINGS:
            assert np.array_equal(a3, acc) and s3.tobytes() == strings.tobytes()
        else:
            assert len(s3) == 0 and all(np.array_equal(a3[f], acc[f]) for f in names)
        assert t3.tobytes() == table.tobytes() and i3.tobytes() == ident.tobytes() and np.array_equal(b3, begin) and nj3 == njobs
    monkeypatch.delenv("MECAT_CNS_SLICE_JOBS")
    # a template without candidates in the middle of the batch: an empty table range, everything behind it one template further
    tb = np.concatenate([g["tb"][:21], g["tb"][20:]])
    a4, s4, nj4, t4, i4, b4 = run_ex(ctx, g, M.CNS_WANT_STRINGS | M.CNS_WANT_TABLE, tb=tb)
    assert b4[20] == b4[21] and np.array_equal(np.delete(b4, 21), begin)
    assert t4.tobytes() == table.tobytes() and i4.tobytes() == ident.tobytes() and s4.tobytes() == strings.tobytes()
    assert np.array_equal(a4["template_index"], acc["template_index"] + (acc["template_index"] >= 20))
    # nothing asked for, or something unknown
    for want in (0, 4):
        with pytest.raises(M.MhipError, match="want"):
            run_ex(ctx, g, want)


def test_the_old_entry_point_is_untouched(ctx, both):
    import mecat_amd.hip as M
    g = golden_subset("pacbio")
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], 0)
    acc0, str0, nj0 = M.cns_accept_templates(ctx, vol, g["pac"], g["cands"].copy(), g["tb"], g["tech"], g["mas"], g["ratio"], threads=16)
    vol.free()
    a1, s1, nj1, t1, i1, b1 = run_ex(ctx, g, M.CNS_WANT_STRINGS)
    assert len(t1) == 0 and len(i1) == 0 and len(b1) == 0
    for acc, strings, nj in ((a1, s1, nj1), both["pacbio"][:3]):
        assert np.array_equal(acc0, acc) and bytes(str0) == strings.tobytes() and nj0 == nj


# ---- against the compiled reference: tests/golden/cns_table.npz ---------------------------------------------------------------------
FULL = {"pacbio": 240, "nanopore": 160}


@pytest.mark.parametrize("name", sorted(FULL))
def test_whole_golden_table_equals_the_reference(ctx, name):
    """every template of the golden accept sets, CNS_WANT_TABLE alone: table and ident bytes are what the unmodified
    consensus_one_read_can_* left in ConsensusThreadData::cns_table and what identify_one_consensus_item makes of it.  No restatement."""
    import mecat_amd.hip as M
    T = TG.golden()
    n = FULL[name]
    g = golden_subset(name, n)
    assert g["K"] == n == len(g["lens"]) == len(T[name + "_table_sha"]) == len(T[name + "_ident_sha"])
    acc, strings, njobs, table, ident, begin = run_ex(ctx, g, M.CNS_WANT_TABLE)
    assert len(strings) == 0 and len(begin) == n + 1 and begin[0] == 0 and len(table) == len(ident) == begin[n]
    assert np.array_equal(np.diff(begin), np.where(np.diff(g["tb"]) > 0, g["lens"], 0))
    bad = []
    for t in range(n):
        if begin[t + 1] == begin[t]:
            assert str(T[name + "_table_sha"][t]) == "" and str(T[name + "_ident_sha"][t]) == "", t      # no candidates, no table
            continue
        if (hashlib.sha256(table[begin[t]: begin[t + 1]].tobytes()).hexdigest() != str(T[name + "_table_sha"][t])
                or hashlib.sha256(ident[begin[t]: begin[t + 1]].tobytes()).hexdigest() != str(T[name + "_ident_sha"][t])):
            bad.append(t)
    b8 = T[name + "_begin8"]
    want_t, want_i = TG.planes_to_table(T[name + "_table8"]), T[name + "_ident8"]
    assert np.array_equal(begin[:9], b8)
    got_t, got_i = table[: b8[8]], ident[: b8[8]]
    for f in R.TABLE_DTYPE.names:
        assert np.array_equal(got_t[f], want_t[f]), (f, np.nonzero(got_t[f] != want_t[f])[0][:10])
    assert np.array_equal(got_i, want_i), np.nonzero(got_i != want_i)[0][:10]
    assert not bad, bad[:10]
    assert int((np.diff(begin) > 0).sum()) == n          # every template of the set has a table: 240 + 160


def test_ident_sweep_on_the_device(ctx):
    """One hook call whose table holds every (mat, ins, del) with mat + ins <= 100 and del <= mat + ins once (348 551 positions, 100
    alignments): positions sorted by cov = mat + ins descending; alignment a spans the positions with cov > a; at position p it has a
    match column if a < mat[p], else an insertion column, and if a < del[p] one query base over a template gap behind it.  Counts must be
    the intended ones, ident the compiled identify_one_consensus_item's (cns_table.npz sweep_ident), base the template letter exactly
    where mat > 0.  Pins comparisons, thresholds and cov == 0, not rounding: over this domain double, float32 and exact integer
    arithmetic agree."""
    import mecat_amd.hip as M
    tri = R.sweep_triples()
    want_id = TG.golden()["sweep_ident"]
    assert len(tri) == len(want_id) == 348551
    cov = tri[:, 0] + tri[:, 1]
    order = np.argsort(-cov, kind="stable")
    mat, ins, dele = (np.ascontiguousarray(x) for x in tri[order].T)
    covs = cov[order]
    rng = np.random.default_rng(9)
    tmpl = LET[rng.integers(0, 4, len(tri))]
    alns = []
    for a in range(R.MAX_CNS_OVLPS):
        P = int((covs > a).sum())
        m, d = a < mat[:P], a < dele[:P]
        ncol = 1 + d.astype(np.int64)
        at = np.cumsum(ncol) - ncol
        q = np.full(int(ncol.sum()), R.GAP, dtype=np.uint8)
        s = np.full(len(q), R.GAP, dtype=np.uint8)
        s[at] = tmpl[:P]
        q[at[m]] = tmpl[:P][m]
        q[at[d] + 1] = LET[a % 4]
        alns.append((q, s, 0))
    assert len(alns[0][0]) > len(tri) and len(alns[-1][0]) >= 101
    table, ident = M.debug_cns_table(ctx, *lay_out(alns), tmpl.tobytes())
    for f, want in (("mat_cnt", mat), ("ins_cnt", ins), ("del_cnt", dele), ("base", np.where(mat > 0, tmpl, ord("N")))):
        assert np.array_equal(table[f], want), (f, np.nonzero(table[f] != want)[0][:10])
    assert np.array_equal(ident, want_id[order]), tri[order][np.nonzero(ident != want_id[order])[0][:10]]
    assert int((covs == 0).sum()) == 1 and np.all(ident[covs == 0] == 7)


def test_adversarial_pairs_equal_the_reference(ctx):
    """every adversarial pair of cns_table.npz through the hook, each on a span of its own of a shared template: [guard][tmpl_len
    positions][guard], as the harness laid the reference's table out, so that the whole block, guards included, must equal what
    meap_add_one_aln left.  A pair with a run of template gaps in front of its first template base at soff == 0 goes to position 0 of a
    call instead (one per call): there the device's table equals the reference's inside the array, and the reference's stray count is in
    its front guard only.  Four leads shift the strings against the 64-byte grid, as test_gpu_cns_strings.py lays pushgaps.npz out."""
    import mecat_amd.hip as M
    pairs = TG.adversarial_pairs()
    letters = [TG.template_of(s, soff, tl) for _, s, soff, tl, _ in pairs]
    lead_run = [TG.leading_run(q, s) for q, s, _, _, _ in pairs]
    zero = [i for i, p in enumerate(pairs) if p[2] == 0 and lead_run[i][0]]
    rest = [i for i, p in enumerate(pairs) if not (p[2] == 0 and lead_run[i][0])]
    ncalls = max(len(zero), -(-len(rest) // 254))
    assert len(zero) >= 50 and len(pairs) >= 900 and sum(1 for i in zero if lead_run[i][1]) >= 20
    strays = 0
    for lead in (0, 1, 7, 13):
        for c in range(ncalls):
            members = ([zero[c]] if c < len(zero) else []) + rest[c::ncalls]
            assert len(members) <= 255
            alns, where, tmpl = [], [], []
            pos = 0
            for i in members:
                q, s, soff, tl, _ = pairs[i]
                at_zero = c < len(zero) and i == zero[c]
                if not at_zero:
                    tmpl.append(LET[:1])            # the front guard's position
                    pos += 1
                alns.append((q, s, pos + soff))
                where.append(pos)
                tmpl += [letters[i], LET[:1]]       # ... and the back guard's
                pos += tl + 1
            tmpl = np.concatenate(tmpl)
            assert len(tmpl) == pos
            table, _ = M.debug_cns_table(ctx, *lay_out(alns, lead), tmpl.tobytes())
            for i, w in zip(members, where):
                q, s, soff, tl, want = pairs[i]
                if w == 0:                          # the pair at position 0: no index -1 on the device
                    assert table[: tl + 1].tobytes() == want[1:].tobytes(), (lead, i)
                    assert int(want[0]["del_cnt"]) == (1 if lead_run[i][1] else 0) and want[0]["mat_cnt"] == want[0]["ins_cnt"] == 0, i
                    strays += int(want[0]["del_cnt"])
                else:
                    got = table[w - 1: w + tl + 1]
                    assert got.tobytes() == want.tobytes(), (lead, i, np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0][:10])
    assert strays >= 4 * 20


def test_volume_whose_first_read_id_is_not_zero(ctx, both):
    """read ids are volume-wide numbers (include/mecat_hip.h: local index = id - start_read_id): the same reads as a volume that starts
    at read 70 001, candidates shifted by as much, give the same bytes — cns_table_finish looks the template's letters up by sid - start"""
    import mecat_amd.hip as M
    start = 70001
    for name in sorted(SUBSET):
        g = golden_subset(name)
        acc, strings, njobs, table, ident, begin = both[name]
        cands = g["cands"].copy()
        cands[:, 1] += start
        cands[:, 7] += start
        a2, s2, nj2, t2, i2, b2 = run_ex(ctx, g, M.CNS_WANT_STRINGS | M.CNS_WANT_TABLE, cands=cands, start_id=start)
        assert t2.tobytes() == table.tobytes() and i2.tobytes() == ident.tobytes() and np.array_equal(b2, begin)
        assert s2.tobytes() == strings.tobytes() and nj2 == njobs
        assert np.array_equal(a2["qid"], acc["qid"] + start) and np.array_equal(a2["sid"], acc["sid"] + start)
        assert all(np.array_equal(a2[f], acc[f]) for f in acc.dtype.names if f not in ("qid", "sid"))
        assert (table["mat_cnt"] > 0).sum() > 1000 and len(set(table["base"][table["mat_cnt"] > 0].tolist())) == 4
