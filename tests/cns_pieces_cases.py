"""Inputs for the piece tests (test_cns_pieces_ref_cpu.py, test_gpu_cns_pieces.py): hand-computed cases of
CnsAln::retrieve_aln_subseqs, a seeded random generator of (alignments, window list) cases, and the census of the situations a set of
cases puts the cursor in — taken from the literal restatement's own output.  An alignment is (qaln, saln, soff, send)."""
import numpy as np

import cns_pieces_ref as Q

GAP = Q.GAP


def aln(saln, soff, qaln=None):
    """an alignment from its template string: send as add_aln gets it (soff + the template bases the string holds); the query string
    repeats the template's letters and puts a T under its gaps unless given"""
    s = saln.encode()
    q = qaln.encode() if qaln is not None else bytes(c if c != GAP else ord("T") for c in s)
    assert len(q) == len(s)
    return q, s, soff, soff + sum(c != GAP for c in s)


FIVE = aln("ACGTA", 10)                      # columns 0..4 at positions 10..14, send 15
# name -> (alignments, windows, pieces by hand (aln, col, ncols, sb_out), piece_begin by hand)
HAND = {
    "starts inside a window: sb_out = soff0 > sb": ([FIVE], [(8, 12)], [(0, 0, 3, 10)], [0, 1]),
    "ends inside a window: clipped at n - 1": ([FIVE], [(12, 20)], [(0, 2, 3, 12)], [0, 1]),
    "ends exactly on se, and is spent for the window that starts there": ([FIVE], [(12, 14), (14, 16)], [(0, 2, 3, 12)], [0, 1, 1]),
    "sb == send - 1 behind a clean stretch: one column": ([FIVE], [(14, 16)], [(0, 4, 1, 14)], [0, 1]),
    "sb == send - 1 behind a listed window that ended in front of it: still one column": ([FIVE], [(11, 13), (14, 16)], [(0, 1, 3, 11), (0, 4, 1, 14)], [0, 1, 2]),
    "se == soff0 is false and leaves the cursor alone": ([FIVE], [(5, 10), (10, 12)], [(0, 0, 3, 10)], [0, 0, 1]),
    "sb >= send": ([FIVE], [(15, 18), (20, 21)], [], [0, 0, 0]),
    "n == 1 never answers": ([aln("A", 3)], [(2, 5)], [], [0, 0]),
    "n == 2": ([aln("AC", 3)], [(2, 5)], [(0, 0, 2, 3)], [0, 1]),
    "n == 2, spent after its first window": ([aln("AC", 3)], [(3, 4), (4, 6)], [(0, 0, 2, 3)], [0, 1, 1]),
    # saln[0] a gap: column 0 still has position soff0, the first base (column 1) soff0 + 1
    "saln[0] a gap": ([aln("-AC-G", 10, "TACTG")], [(10, 12), (12, 13)], [(0, 0, 3, 10), (0, 2, 3, 12)], [0, 1, 2]),
    # gap columns behind the base at se stay out of the piece; the last window takes them to the end
    "trailing gap columns": ([aln("ACG--", 0)], [(1, 2), (2, 5)], [(0, 1, 2, 1), (0, 2, 3, 2)], [0, 1, 2]),
    "gap runs inside windows": ([aln("AC--GT-A", 0)], [(0, 2), (2, 3), (3, 4)], [(0, 0, 5, 0), (0, 4, 2, 2), (0, 5, 3, 3)], [0, 1, 2, 3]),
    "a gap run behind se belongs to the next window": ([aln("AC--GT-A", 0)], [(0, 1), (1, 2)], [(0, 0, 2, 0), (0, 1, 4, 1)], [0, 1, 2]),
    "add order, one alignment without a part": ([FIVE, aln("A-CG", 11), aln("ACGT", 20)], [(11, 13)], [(0, 1, 3, 11), (1, 0, 4, 11)], [0, 2]),
    "no window": ([FIVE], [], [], [0]),
    "no alignment": ([], [(1, 2)], [], [0, 0]),
}


def random_windows(rng, L, dense):
    """ascending, disjoint (sb, se) in [0, L]; `dense`: most windows touch the one in front"""
    out = []
    p = int(rng.integers(0, 4))
    while True:
        p += int(rng.choice([0, 0, 0, 1, 2, 7])) if dense else int(rng.choice([0, 1, 3, 9, 30]))
        se = p + int(rng.choice([1, 1, 2, 3, 5, 12]))
        if se > L:
            return out
        out.append((p, se))
        p = se


def random_aln(rng, L, windows, max_bases):
    """one alignment on a template of L positions, its ends often on a window's boundary"""
    edges = [e for w in windows for e in w] or [0]
    pick = lambda: int(rng.choice(edges)) + int(rng.choice([-1, 0, 0, 0, 1]))
    soff = pick() if rng.random() < 0.5 else int(rng.integers(0, L))
    soff = min(max(soff, 0), L - 1)
    nb = int(rng.integers(1, max_bases + 1))
    if rng.random() < 0.5:
        nb = pick() - soff
    nb = min(max(nb, 1), L - soff, max_bases)
    if rng.random() < 0.06:
        nb = int(rng.choice([1, 2]))
    pg = float(rng.choice([0.0, 0.05, 0.2, 0.5]))
    s = bytearray()
    if rng.random() < 0.1:
        s += b"-" * int(rng.integers(1, 3))                   # saln[0] a gap
    for i in range(nb):
        if i and rng.random() < pg:
            s += b"-" * int(rng.choice([1, 1, 2, 3, 70]) if max_bases > 200 else rng.choice([1, 1, 2, 3]))
        s.append(int(rng.choice(list(b"ACGT"))))
    if rng.random() < 0.15:
        s += b"-" * int(rng.integers(1, 4))                   # trailing gap columns
    q = bytearray(s)
    for i, c in enumerate(s):
        if c == GAP:
            q[i] = ord("T") if rng.random() < 0.95 else GAP
        elif rng.random() < 0.1:
            q[i] = GAP
    return bytes(q), bytes(s), soff, soff + nb


def random_case(rng, L, max_alns, max_bases):
    windows = random_windows(rng, L, rng.random() < 0.7)
    return [random_aln(rng, L, windows, max_bases) for _ in range(int(rng.integers(1, max_alns + 1)))], windows


SITUATIONS = ("starts_inside", "clipped", "ends_on_se", "se_eq_soff", "last_base_one_column", "last_base_spent", "sb_ge_send", "n1", "n2_piece", "lead_gap_piece",
              "trailing_gap_piece", "gap_inside", "gap_behind_first_column")


def census(alns, windows, pieces, piece_begin, count):
    """adds the situations of one case to `count` (a dict over SITUATIONS), read off the pieces `retrieve_literal` returned"""
    have = {}
    for w in range(len(windows)):
        for p in pieces[piece_begin[w]: piece_begin[w + 1]]:
            have[int(p["aln"]), w] = p
    for k, (q, s, soff, send) in enumerate(alns):
        n = len(s)
        pos = Q.column_positions(s, soff)
        count["n1"] += n == 1 and len(windows) > 0
        for w, (sb, se) in enumerate(windows):
            p = have.get((k, w))
            count["se_eq_soff"] += se == soff and p is None
            count["sb_ge_send"] += sb >= send and p is None
            plain_end = n >= 2 and s[0] != GAP and s[n - 1] != GAP and sb == send - 1
            count["last_base_one_column"] += plain_end and p is not None and int(p["ncols"]) == 1 and int(p["col"]) == n - 1
            count["last_base_spent"] += plain_end and p is None and w > 0 and windows[w - 1][1] == sb and windows[w - 1][1] > soff
            if p is None:
                continue
            col, last = int(p["col"]), int(p["col"]) + int(p["ncols"]) - 1
            count["starts_inside"] += int(p["sb_out"]) > sb
            count["clipped"] += last == n - 1 and pos[n - 1] < se
            count["ends_on_se"] += last == n - 1 and pos[n - 1] == se
            count["n2_piece"] += n == 2
            count["lead_gap_piece"] += s[0] == GAP
            count["trailing_gap_piece"] += s[n - 1] == GAP and last == n - 1
            count["gap_inside"] += GAP in s[col + 1: last]
            count["gap_behind_first_column"] += col > 0 and last > col and s[col + 1] == GAP
