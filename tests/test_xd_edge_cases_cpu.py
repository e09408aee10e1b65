"""The inputs of tests/xd_edge_cases.py, on the CPU: the oracle equals the compiled reference on exactly these inputs (low-complexity
sequence and periodic substitutions are outside what tests/test_oracle_vs_ref.py's random draws pin), the walker's chaining equals
orc_xdrop_go, and every family meets the premises it was built for.  The GPU tests (test_gpu_xalign_edges.py,
test_gpu_ref_xextend_edges.py) rely on those premises: a generated case that misses one fails here, it is not dropped."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import xd_edge_cases as E

NAMES = "ABCDE"
needs_ref = pytest.mark.skipif(not H.ref_available(), reason="oracle/_ref not built")


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_compiled_reference_on_these_blocks_and_jobs(name):
    """every block of every unit through refh_xdrop_align and orc_xdrop_align (score, end point, edit block), and the traced call gives the
    same block; every job through refh_xdrop_go and orc_xdrop_go.  A start point in front of a read is left out of the second: the
    reference reads in front of its arrays there, and the product does not extend such a job (tests/test_gpu_parity.py)."""
    R, O = H.ref(), H.orc()
    f = E.family(name)
    nblk = 0
    for b in f.blocks():
        if b["M"] <= 0 or b["N"] <= 0:
            continue
        outs = []
        for fn, pre in ((R.refh_xdrop_align, ()), (O.orc_xdrop_align, (E.xaligner(),))):
            res = np.zeros(3, np.int32)
            ops = np.zeros(2 * (b["M"] + b["N"] + 2), np.int32)
            sc = fn(*pre, b["q"].ctypes.data, b["M"], b["t"].ctypes.data, b["N"], b["forward"], res.ctypes.data, ops.ctypes.data)
            outs.append((sc, tuple(res), tuple(ops[: 2 * res[2]])))
        assert outs[0] == outs[1], (name, nblk)
        assert (b["ae"], b["be"], tuple(b["ops"])) == (outs[1][1][0], outs[1][1][1], outs[1][2]), (name, nblk)
        nblk += 1
    njobs = 0
    for q, t, qs, ts, lab in f.pairs:
        if qs < 0 or ts < 0:
            continue
        qc, tc = np.ascontiguousarray(q), np.ascontiguousarray(t)
        res_r = np.zeros(7, dtype=np.int32)
        ident = C.c_double()
        R.refh_xdrop_go(qc.ctypes.data, qs, len(qc), tc.ctypes.data, ts, len(tc), 1, res_r.ctypes.data, C.byref(ident))
        assert E.go(q, qs, t, ts, 1) == tuple(int(x) for x in res_r), (name, lab)
        njobs += 1
    print("family %s: %d blocks and %d jobs equal the compiled reference" % (name, nblk, njobs))
    assert nblk > 100 and njobs > 100


@pytest.mark.parametrize("name", NAMES)
def test_the_walker_equals_orc_xdrop_go(name):
    f = E.family(name)
    for (q, t, qs, ts, lab), w in zip(f.pairs, f.walks()):
        for min_aln in (1, 500):
            assert E.result_tuple(w, min_aln) == E.go(q, qs, t, ts, min_aln), (name, lab)
        a, b = E.strings(w)
        assert len(a) == len(b) == w["res"]["columns"]
    tot = f.totals()
    print("family %s: %s" % (name, tot))
    assert max(len(u) for _, _, u in f.units()) <= 8          # (few blocks per unit: the GPU tests stay quick)


def single_blocks(f):
    """families A and B: the left half is empty, the right half one last block"""
    out = []
    for (q, t, qs, ts, lab), w in zip(f.pairs, f.walks()):
        assert (qs, ts) == (0, 0) and len(w["left"]) == 1 and w["left"][0]["rows"] == 0
        assert len(w["right"]) == 1 and w["right"][0]["last"]
        b = w["right"][0]
        assert (b["qblk"], b["tblk"]) == (min(len(q), int(len(t) * 1.2)), min(len(t), int(len(q) * 1.2)))
        out.append((lab, b))
    return out


def test_family_a_window_ladder():
    f = E.family("A")
    blocks = single_blocks(f)
    widest = sorted(set(b["widest"] for _, b in blocks))
    print("family A: widest windows", widest)
    for w in list(range(62, 68)) + list(range(124, 130)):
        assert w in widest, w
    # the construction: 47 + k cells, in steps of one, so the ring's limit lies between k = 79 and k = 80
    for (k, mirrored), b in blocks:
        if not mirrored:
            assert b["widest"] == 47 + k, (k, b["widest"])
    assert sum(b["widest"] == 126 for _, b in blocks) >= 2 and sum(b["widest"] == 127 for _, b in blocks) >= 2
    # both sides of the one-pass / two-pass edge: a window of exactly 64 cells and one of 65
    assert 64 in widest and 65 in widest


def test_family_b_traceback_in_the_second_chunk():
    f = E.family("B")
    blocks = single_blocks(f)
    n_hi = n_gap = n_over = 0
    for lab, b in blocks:
        hi = b["idx"] >= 64
        if b["widest"] <= E.RING_CELLS and int(hi.sum()) >= 30:
            n_hi += 1
            n_gap += int((hi & b["gap"]).any())
        n_over += b["widest"] > E.RING_CELLS
        assert b["ae"] >= b["qblk"] - 20 or b["be"] >= b["tblk"] - 20, lab          # the best cell lies behind the stretch
    print("family B: %d ring blocks with >= 30 path cells at window index >= 64, %d of them with a gap step there; %d blocks outgrow the ring"
          % (n_hi, n_gap, n_over))
    assert n_hi >= 10 and n_gap >= 1


def test_family_c_tail_patterns_and_trim_edges():
    f = E.family("C")
    acnt, kinds, trims = set(), {}, {}
    shown = {(k, d): 0 for k in "MSQT" for d in (0, 1)}          # units that end with what block 1 kept, by the column in front of its tail
    row15 = 0
    for j, d, bl in f.units():
        lab = f.pairs[j][4]
        if d != lab[-1]:
            continue          # (the other half: empty, or the 50 bases behind a left start point)
        b = bl[0]
        assert (b["qblk"], b["tblk"]) == (500, 500) and not b["last"] and b["full_map"], lab
        if lab[0] == "tail":
            assert b["trim_ok"], lab
            acnt.add(b["acnt"])
            kinds.setdefault(b["l1"], set()).add(b["acnt"])
            # block 2's only run of four matches is block 1's, at its very first columns: refused, the direction ends with block 1's kept part
            ends_there = len(bl) == 2 and bl[1]["full_map"] and not bl[1]["last"] and bl[1]["found"] and bl[1]["kept"] == 0
            if lab[3] == "equal":
                assert len(bl) >= 2 and bl[1]["used"], lab
            elif ends_there:
                shown[b["l1"], d] += 1
                # the ring's traceback takes 32 columns in its first turn: from a row that is 15 modulo 16, no gap and no run of four in them
                row15 += b["ae"] % 16 == 15 and not b["gap"][:32].any() and b["acnt"] > 32
        else:
            trims.setdefault(d, {})[lab[1]] = (b["found"], b["kept"], b["trim_ok"])
    print("family C: units that end with block 1's kept part, by (column in front of the tail, direction):", shown, "; first turns of 32 columns:", row15)
    # (a query-only column in front of the tail comes from one pattern at 71 positions: at least half of them must show, in either direction)
    assert min(shown.values()) >= 36 and row15 >= 40
    print("family C: acnt values %d..%d, missing below 71: %s" % (min(acnt), max(acnt), [x for x in range(4, 71) if x not in acnt]))
    # The issue asks for every acnt from 5 to 70.  5 and 6 cannot occur: a block's end point is the FIRST cell with the best score, so its last
    # column is a match, and so is the one before it unless the two cancel (a non-match and a match end where the path stood two columns
    # earlier, in a cell visited before).  The tail is therefore MMMM (acnt 4) or starts with two matches and a non-match (acnt >= 7).
    assert 5 not in acnt and 6 not in acnt
    for x in [4] + list(range(7, 71)):
        assert x in acnt, x
    for kind in "MSQT":
        v = kinds[kind]
        spread = (sum(x < 32 for x in v), sum(32 <= x <= 64 for x in v), sum(x > 64 for x in v))
        print("family C: column %s in front of the trimmed tail: acnt below 32 / in 32..64 / above 64: %s" % (kind, spread))
        assert min(spread) >= 1, (kind, spread)
    print("family C: trim edges (found, n - acnt, trim_ok) by direction:", trims)
    for d in (0, 1):
        assert trims[d] == {0: (True, 0, False), 1: (True, 1, False), 2: (True, 2, True), 3: (True, 3, True), None: (False, 0, False)}, trims[d]


def test_family_d_block_geometry():
    f = E.family("D")
    qside, tside, qrest, trest, small_n, small_m = set(), set(), set(), set(), set(), set()
    for j, d, bl in f.units():
        lab = f.pairs[j][4]
        qside.add((bl[0]["qleft"], d)); tside.add((bl[0]["tleft"], d))
        for b in bl:
            if not b["last"]:
                qrest.add((b["qblk"] - b["ae"], b["full_map"])); trest.add((b["tblk"] - b["be"], b["full_map"]))
            small_n.add(b["N"]); small_m.add(b["M"])
        if lab[0] == "negative":
            assert len(bl) == 1 and bl[0]["rows"] == 0
    for d in (0, 1):
        for s in E.D_SIDES:
            assert (s, d) in qside and (s, d) in tside, (s, d)
        for s in E.D_TARGET_SIDES:
            assert (s, d) in tside, (s, d)
        for s in E.D_QUERY_SIDES:
            assert (s, d) in qside, (s, d)
    for n in E.D_TARGET_SIDES:
        assert n in small_n, n          # the block's own N: rows of the N <= 30 code and the first sizes beyond it
    for m in E.D_QUERY_SIDES:
        assert m in small_m, m
    # full_map is `qblk - ae <= 20 || tblk - be <= 20`: 20 on either side alone maps the block, 21 on both does not
    for want in ((20, True), (21, True), (21, False)):
        assert want in qrest and want in trest, want
    print("family D: side lengths", sorted(s for s, _ in qside if s in E.D_SIDES + E.D_QUERY_SIDES), sorted(s for s, _ in tside if s in E.D_SIDES + E.D_TARGET_SIDES),
          "; qblk - ae", sorted(x for x, _ in qrest if 18 <= x <= 23), "tblk - be", sorted(x for x, _ in trest if 18 <= x <= 23))
    assert f.totals()["redone"] == 0


def test_family_e_overflow_behind_the_first_block():
    f = E.family("E")
    st = {(what, d): 0 for what in ("units", "later", "two", "ring_behind") for d in (0, 1)}
    for j, d, bl in f.units():
        ov = [i for i, b in enumerate(bl) if b["widest"] > E.RING_CELLS]
        if ov:
            st["units", d] += 1
            st["later", d] += ov[0] >= 1
            st["two", d] += len(ov) >= 2
            st["ring_behind", d] += len(bl) - 1 > ov[-1]
    print("family E: units with a block that outgrows the ring, by direction (0 = left):", st)
    for d in (0, 1):
        assert st["later", d] >= 10 and st["ring_behind", d] >= 10, st
    assert st["two", 0] + st["two", 1] >= 10, st
    assert f.totals()["wide_units"] == st["units", 0] + st["units", 1]


def test_families_without_a_wide_block():
    """the counters of the default arrangement are compared on these: no block is redone"""
    assert E.family("C").totals()["redone"] == 0 and E.family("D").totals()["redone"] == 0
    low = E.ladder_below()
    assert low.totals()["redone"] == 0 and len(low.jobs) >= 60
    assert max(b["widest"] for b in low.blocks()) == E.RING_CELLS
