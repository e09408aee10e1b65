"""The restatements of CnsAln::retrieve_aln_subseqs (tests/cns_pieces_ref.py) against hand-computed pieces and against each other, and
the C ABI of the piece entry points.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cns_pieces_cases as K
import cns_pieces_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(K.HAND))
def test_hand_computed(name):
    alns, windows, pieces, piece_begin = K.HAND[name]
    want = Q.as_arrays(pieces, piece_begin)
    assert Q.same_pieces(Q.retrieve_literal(alns, windows), want) is None, Q.same_pieces(Q.retrieve_literal(alns, windows), want)
    assert Q.same_pieces(Q.pieces_closed_form(alns, windows), want) is None, Q.same_pieces(Q.pieces_closed_form(alns, windows), want)


def test_the_literal_cursor_returns_the_substrings():
    """the strings the cursor collects are the column range the piece names, gap columns included"""
    q, s, soff, send = K.aln("AC--GT-A", 0, "ACTTG-TA")
    a = Q.CnsAln(soff, send, q, s)
    assert a.retrieve_aln_subseqs(0, 2) == (b"ACTTG", b"AC--G", 0, 0)
    assert a.retrieve_aln_subseqs(2, 3) == (b"G-", b"GT", 2, 4)
    assert a.retrieve_aln_subseqs(3, 9) == (b"-TA", b"T-A", 3, 5)
    assert a.retrieve_aln_subseqs(9, 12) is None and (a.aln_idx, a.soff) == (7, 4)


# what the 20 000 cases must contain, per situation of cns_pieces_cases.SITUATIONS; seed 20261 meets it (the counts it gives are far above)
NEED = dict(starts_inside=2000, clipped=2000, ends_on_se=500, se_eq_soff=500, last_base_one_column=100, last_base_spent=100, sb_ge_send=2000, n1=200, n2_piece=200,
            lead_gap_piece=1000, trailing_gap_piece=300, gap_inside=2000, gap_behind_first_column=500)


def test_closed_form_is_the_literal_cursor():
    rng = np.random.default_rng(20261)
    count = dict.fromkeys(K.SITUATIONS, 0)
    npieces = 0
    for case in range(20000):
        alns, windows = K.random_case(rng, int(rng.integers(4, 70)), 4, 40)
        lit = Q.retrieve_literal(alns, windows)
        got = Q.pieces_closed_form(alns, windows)
        assert Q.same_pieces(got, lit) is None, (case, Q.same_pieces(got, lit), alns, windows)
        K.census(alns, windows, lit[0], lit[1], count)
        npieces += len(lit[0])
    print({k: int(v) for k, v in count.items()}, npieces)
    assert npieces >= 40000          # two pieces per case on average: the cases are not mostly empty
    for k, v in NEED.items():
        assert count[k] >= v, (k, int(count[k]), v)


def test_abi():
    """libmecat_hip.so exports the two entry points, and a piece is 16 bytes in C as in numpy"""
    import mecat_amd.hip as M
    L = C.CDLL(M.lib_path())
    assert L.mhip_cns_accept_templates_pieces and L.mhip_debug_cns_pieces
    assert M.PIECE_DTYPE == Q.PIECE_DTYPE and M.PIECE_DTYPE.itemsize == 16 and M.CNS_WANT_PIECES == 8
    src = '#include "mecat_hip.h"\n_Static_assert(sizeof(mhip_cns_piece) == 16, "piece");\n_Static_assert(MHIP_CNS_WANT_PIECES == 8, "bit");\n'
    r = subprocess.run(["cc", "-x", "c", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
