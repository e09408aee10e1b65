"""tests/cns_table_ref.py — the restatement of the consensus table rules that test_gpu_cns_table.py holds the device against — pinned
to LITERAL tables worked out by hand from those rules (meap_add_one_aln / identify_one_consensus_item of mecat2cns), so that the
checker itself is checked.  Template "ACGTACGTAC"; rows below are (mat, ins, del) per template position.

Below those, the restatement is held against the COMPILED, UNMODIFIED reference (oracle/_ref/libref_cns_table.so, results recorded in
tests/golden/cns_table.npz by tests/golden/make_golden_cns_table.py): meap_add_one_aln on 1 060 adversarial pairs,
identify_one_consensus_item on every count triple a table position can hold; and, where oracle/_ref is built, the fixture is regenerated
from the harness."""
import hashlib

import numpy as np
import pytest

import cns_table_golden as TG
import cns_table_ref as R
import helpers as H

T = b"ACGTACGTAC"
Z = (0, 0, 0)


def table_of(alns):
    t, ident = R.build_table(alns, T)
    return [(int(a), int(b), int(c)) for a, b, c in zip(t["mat_cnt"], t["ins_cnt"], t["del_cnt"])], bytes(t["base"]), ident.tolist()


CASES = {
    # q, s, soff -> rows 0..9
    "match": ((b"GTA", b"GTA", 2), [Z, Z, (1, 0, 0), (1, 0, 0), (1, 0, 0), Z, Z, Z, Z, Z]),
    "insertion": ((b"G-A", b"GTA", 2), [Z, Z, (1, 0, 0), (0, 1, 0), (1, 0, 0), Z, Z, Z, Z, Z]),
    "deletion": ((b"GCT", b"G-T", 2), [Z, Z, (1, 0, 1), (1, 0, 0), Z, Z, Z, Z, Z, Z]),
    "s-gap run of 3 counts once": ((b"GCCCT", b"G---T", 2), [Z, Z, (1, 0, 1), (1, 0, 0), Z, Z, Z, Z, Z, Z]),
    "double gap in front of the run's base": ((b"G-CT", b"G--T", 2), [Z, Z, (1, 0, 1), (1, 0, 0), Z, Z, Z, Z, Z, Z]),
    "double gap inside the run": ((b"GC-CT", b"G---T", 2), [Z, Z, (1, 0, 1), (1, 0, 0), Z, Z, Z, Z, Z, Z]),
    "double gap alone": ((b"G-T", b"G-T", 2), [Z, Z, (1, 0, 0), (1, 0, 0), Z, Z, Z, Z, Z, Z]),
    "run at the very start, soff > 0": ((b"CGT", b"-GT", 2), [Z, (0, 0, 1), (1, 0, 0), (1, 0, 0), Z, Z, Z, Z, Z, Z]),
    "run at the very start, soff == 0": ((b"GAC", b"-AC", 0), [(1, 0, 0), (1, 0, 0), Z, Z, Z, Z, Z, Z, Z, Z]),
    "two runs, one base apart": ((b"GCTCA", b"G-T-A", 2), [Z, Z, (1, 0, 1), (1, 0, 1), (1, 0, 0), Z, Z, Z, Z, Z]),
    "insertion then deletion": ((b"G-CA", b"GT-A", 2), [Z, Z, (1, 0, 0), (0, 1, 1), (1, 0, 0), Z, Z, Z, Z, Z]),
    "run at the end": ((b"ACTT", b"AC--", 8), [Z, Z, Z, Z, Z, Z, Z, Z, (1, 0, 0), (1, 0, 1)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_tally_of_one_pair(name):
    aln, want = CASES[name]
    rows, base, _ = table_of([aln])
    assert rows == want
    assert base == bytes(T[i] if r[0] else ord("N") for i, r in enumerate(want))


def test_pairs_add_up_and_base_is_the_template_letter():
    alns = [CASES[k][0] for k in ("match", "insertion", "deletion", "run at the very start, soff > 0")]
    rows, base, ident = table_of(alns)
    assert rows == [Z, (0, 0, 1), (4, 0, 1), (3, 1, 0), (2, 0, 0), Z, Z, Z, Z, Z]
    assert base == b"NNGTANNNNN"
    # position 2: cov 4, mat 4 >= 3.2, del 1 < 1.6 -> FMAT; position 3: cov 4, mat 3 < 3.2, ins 1 < 3.2 -> UNDS; uncovered: 0 >= 0 thrice -> 7
    assert ident == [7, 7, 1, 8, 1, 7, 7, 7, 7, 7]


def test_a_mismatch_column_is_refused():
    with pytest.raises(ValueError):
        R.build_table([(b"GA", b"GT", 2)], T)


@pytest.mark.parametrize("mat,ins,dele,want", [
    (0, 0, 0, 7),        # cov 0: every comparison is 0 >= 0
    (0, 0, 3, 7),
    (4, 0, 1, 1),        # cov 4: 0.8 cov = 3.2, 0.4 cov = 1.6
    (4, 0, 2, 3),
    (3, 1, 1, 8),
    (3, 1, 2, 10),
    (0, 4, 0, 4),
    (1, 3, 2, 10),
    (4, 1, 1, 1),        # cov 5: 0.8 cov = 4.0 exactly, 0.4 cov = 2.0 exactly
    (4, 1, 2, 3),
    (3, 2, 1, 8),
    (1, 4, 0, 4),
    (1, 4, 2, 6),
    (8, 2, 3, 1),        # cov 10: 8.0 and 4.0
    (8, 2, 4, 3),
    (7, 3, 3, 8),
    (7, 3, 4, 10),
    (2, 8, 0, 4),
    (3, 7, 4, 10),
])
def test_ident(mat, ins, dele, want):
    assert R.ident_of(np.array([mat]), np.array([ins]), np.array([dele])).tolist() == [want]


# ---- against the compiled reference ----------------------------------------------------------------------------------------------------
def test_tally_equals_the_reference_on_the_adversarial_pairs():
    """tally_one / build_table == the reference's meap_add_one_aln on a fresh table, item by item (base included), for the reference's own
    normalize_gaps outputs (pushgaps.npz) and the generated pairs.  Where a run of template gaps with a query base stands in front of the
    first template base at soff == 0, the reference counts one deletion at index -1 (the harness's front guard); the restatement holds
    nothing for it, and everything inside the table is equal all the same."""
    fresh = np.zeros(1, dtype=R.TABLE_DTYPE)
    fresh["base"] = ord("N")
    seen = dict(stray=0, lead0_no_base=0, lead_inside=0, begins_double=0, double_only=0, last_col=0, no_tmpl_base=0)
    pairs = TG.adversarial_pairs()
    for i, (q, s, soff, tmpl_len, want) in enumerate(pairs):
        table, _ = R.build_table([(q, s, soff)], TG.template_of(s, soff, tmpl_len))
        assert table.tobytes() == want[1:-1].tobytes(), (i, np.nonzero(table.view(np.uint32) != want[1:-1].view(np.uint32))[0][:10])
        lead, has_base = TG.leading_run(q, s)
        stray = lead and has_base and soff == 0
        assert want[0].tobytes() == (np.array([(ord("N"), 0, 0, 1)], dtype=R.TABLE_DTYPE) if stray else fresh).tobytes(), i
        assert want[-1].tobytes() == fresh.tobytes(), i
        sg, qg = s == R.GAP, q == R.GAP
        seen["stray"] += stray
        seen["lead0_no_base"] += lead and not has_base and soff == 0
        seen["lead_inside"] += lead and has_base and soff > 0
        seen["begins_double"] += bool(np.any(sg[1:] & qg[1:] & ~sg[:-1]))
        seen["double_only"] += bool(sg.any()) and bool(np.all(qg[sg]))
        seen["last_col"] += bool(sg[-1])
        seen["no_tmpl_base"] += bool(sg.all())
    assert len(pairs) >= 700 + 200 and all(v >= 10 for v in seen.values()), seen


def test_ident_equals_the_reference_on_every_triple_a_position_can_hold():
    """ident_of == the compiled identify_one_consensus_item for every (mat, ins, del) with mat + ins <= 100 (MAX_CNS_OVLPS) and
    del <= mat + ins: 348 551 triples.  This pins the comparisons, the `>=` thresholds 0.8 / 0.4 and the cov == 0 case.  It does NOT pin
    the rounding: over this domain double, float32 and exact integer arithmetic (5 mat >= 4 cov, 5 del >= 2 cov) all give the same byte."""
    tri = R.sweep_triples()
    want = TG.golden()["sweep_ident"]
    assert len(tri) == len(want) == 348551
    assert np.all(tri[:, 0] + tri[:, 1] <= 100) and np.all(tri[:, 2] <= tri[:, 0] + tri[:, 1]) and len(np.unique(tri, axis=0)) == len(tri)
    got = R.ident_of(tri[:, 0], tri[:, 1], tri[:, 2])
    assert np.array_equal(got, want), tri[np.nonzero(got != want)[0][:10]]
    assert want[0] == 7 and sorted(set(want.tolist())) == [1, 3, 4, 6, 7, 8, 10]


@pytest.mark.skipif(not H.ref_cns_table_available(), reason="mecat2cns table harness not built (oracle/_ref)")
def test_the_golden_regenerates_from_the_harness():
    g = TG.golden()
    for name in ("pacbio", "nanopore"):
        res = TG.reference_tables(name, 8)
        b = g[name + "_begin8"]
        stored_t, stored_i = TG.planes_to_table(g[name + "_table8"]), g[name + "_ident8"]
        for t, (_, _, table, ident) in enumerate(res):
            assert hashlib.sha256(table.tobytes()).hexdigest() == str(g[name + "_table_sha"][t]), (name, t)
            assert hashlib.sha256(ident.tobytes()).hexdigest() == str(g[name + "_ident_sha"][t]), (name, t)
            assert table.tobytes() == stored_t[b[t]: b[t + 1]].tobytes() and ident.tobytes() == stored_i[b[t]: b[t + 1]].tobytes(), (name, t)
    assert np.array_equal(TG.reference_sweep(), g["sweep_ident"])
    for i, (q, s, soff, tmpl_len, want) in enumerate(TG.adversarial_pairs()):
        assert TG.reference_add_one(q, s, soff, tmpl_len).tobytes() == want.tobytes(), i
    # the harness refuses what the reference would abort or overrun on, before it calls it
    L = H.ref_cns_table()
    tab, guards = np.zeros(4, dtype=R.TABLE_DTYPE), np.zeros(2, dtype=R.TABLE_DTYPE)
    args = (tab.ctypes.data, 4, guards.ctypes.data)
    assert L.refc_add_one_aln(b"GA", b"GT", 2, 0, *args) == -1
    assert L.refc_add_one_aln(b"GATTA", b"GATTA", 5, 0, *args) == -2 and L.refc_add_one_aln(b"GA", b"GA", 2, 3, *args) == -2
    assert L.refc_add_one_aln(b"GA", b"GA", 2, -1, *args) == -2 and not tab.view(np.uint32).any()
    assert L.refc_add_one_aln(b"GA", b"GA", 2, 2, *args) == 0 and tab["mat_cnt"].tolist() == [0, 0, 1, 1]
    assert L.refc_add_one_aln(b"GA", b"GA", 2, 2, *args) == 0 and tab["mat_cnt"].tolist() == [0, 0, 2, 2]      # calls add up
