"""tests/cns_table_ref.py — the restatement of the consensus table rules that test_gpu_cns_table.py holds the device against — pinned
to LITERAL tables worked out by hand from those rules (meap_add_one_aln / identify_one_consensus_item of mecat2cns), so that the
checker itself is checked.  Template "ACGTACGTAC"; rows below are (mat, ins, del) per template position."""
import numpy as np
import pytest

import cns_table_ref as R

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
