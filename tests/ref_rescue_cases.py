"""Inputs and fixture access shared by the tests of mecat2ref's rescue stage (tests/golden/ref_rescue.npz, made by
tests/golden/make_golden_ref_rescue.py from the unmodified rescue_clipped_align and output_results; the reference is ref_cand.npz's).

A case is a dict: name, read (letters), block_size, bc, num_output, entries [(qoff, qend, qdir, soff, send)] (entry t has id t), and per
strand a database {segment: (score2, loczhi[20], seedno[20])}.  The entries are hand-made, and so are the databases: seeds laid along the
diagonal on which a stretch of the read was copied from the reference, so that the unmodified extension really aligns what the search
finds."""
import json
import os

import numpy as np

import helpers as H
import ref_cand_cases as RC
import ref_cand_ref as R

FIXTURE = os.path.join(H.GOLDEN, "ref_rescue.npz")
SM = 20
AFTER_FIELDS = ("qoff", "qend", "qdir", "soff", "send", "id", "prev_id", "next_id", "parent_id")
NEW_FIELDS = ("vscore", "chain", "qb", "qe", "qs", "sb", "se", "cols", "crc_q", "crc_s")


def bc_of(read_len, rnd):
    return 5 if rnd else min(20, 5 + read_len // 1000)


def diag_segment(q0, p0, seg, block_size, bc, count, stored=None, spoil=0):
    """the record of segment `seg` with `count` seeds on the diagonal read position q <-> 0-based reference position p0 + (q - q0):
    the first query k-mers (stride bc) whose 1-based reference position lies in the segment.  score2 = count, min(count, 20) entries
    stored (or `stored`); the last `spoil` stored entries get a seed number that fits no other (they take no vote)"""
    loc, seed = [], []
    s = max(1, -(-q0 // bc) + 1)
    while len(loc) < min(count, SM) if stored is None else len(loc) < stored:
        q = (s - 1) * bc
        P = p0 + (q - q0) + 1
        if P // block_size > seg:
            break
        if P // block_size == seg:
            loc.append(P % block_size)
            seed.append(s)
        s += 1
    assert len(loc) == (min(count, SM) if stored is None else stored), (seg, len(loc))
    for i in range(spoil):
        seed[len(seed) - 1 - i] = 1 + i          # far off the diagonal, and in falling order: no pair with a later entry
    pad = SM - len(loc)
    return (count, loc + [0] * pad, seed + [0] * pad)


def garbage_segment(count, rng):
    """a record whose seeds agree on no diagonal"""
    return (count, [int(x) for x in rng.permutation(900)[:SM]], [int(x) for x in rng.permutation(300)[:SM] + 1])


def make_cases(U):
    """U: the reference's letters, upper-cased -> the list of cases"""
    G = len(U)
    rng = np.random.default_rng(20263)
    comp = R.revcomp
    cases = []

    def add(name, read, entries, fwd=None, rev=None, rnd=0, num_output=10, bc=None):
        read = np.ascontiguousarray(read, dtype=np.uint8)
        cases.append(dict(name=name, read=read, block_size=2000 if rnd else 1000, bc=bc_of(len(read), rnd) if bc is None else bc, num_output=num_output,
                          entries=[tuple(int(x) for x in e) for e in entries], fwd=fwd or {}, rev=rev or {}))

    # ---- steps 1 to 3 and 7 alone: no segment has a seed, so nothing is rescued
    dummy = np.full(10000, ord("A"), dtype=np.uint8)
    # equal lengths among 10 entries keep their order; none contains another (every one starts 150 further left on the reference)
    ties = [(0, [3000, 2000, 3000, 2500, 2000, 3000, 2500, 1000, 2000, 3000][t], t % 2, 50000 - 150 * t, 50000 - 150 * t + 3000) for t in range(10)]
    add("ties10", dummy, ties)
    for no in (1, 2, 3):
        add("ties10_out%d" % no, dummy, ties, num_output=no)
    # AlignInfoContained: each of the four comparisons at equality (contained) and one off it (kept)
    a = (1000, 5000, 0, 20000, 24000)
    inner = dict(qoff=1500, qend=4500, soff=20500, send=23500)          # well inside a, and shorter: it sorts behind it
    for k, (field, v) in enumerate([("qoff", 900), ("qoff", 899), ("qend", 5100), ("qend", 5101), ("soff", 19900), ("soff", 19899), ("send", 24100),
                                    ("send", 24101)]):
        b = dict(inner, **{field: v})
        assert b["qend"] - b["qoff"] < a[1] - a[0]
        add("contain_%s_%d" % (field, v), dummy, [(b["qoff"], b["qend"], 0, b["soff"], b["send"]), a])
    add("contain_other_strand", dummy, [(1100, 4900, 1, 20100, 23900), a])
    # a chain: the middle entry is removed by the first, so it no longer removes the third
    add("contain_chain", dummy, [(1000, 5000, 0, 20000, 24000), (1050, 4900, 0, 19950, 23900), (1040, 4700, 0, 19870, 23700)])
    add("empty", dummy, [])
    add("one", dummy, [(100, 1200, 1, 300, 1400)])

    # ---- with seeds: reads copied from the reference in two stretches
    def two(a0, n0, a1, n1):
        return np.concatenate([U[a0: a0 + n0], U[a1: a1 + n1]])

    # right attach, forward strand; segments 37 and 38 hold 8 seeds each (the lower index wins on the right), two of segment 38's spoiled
    rd = two(33000, 3000, 36500, 3000)
    bc = bc_of(6000, 0)
    e0 = (0, 3000, 0, 33000, 36000)
    add("right_attach", rd, [e0], fwd={37: diag_segment(3000, 36500, 37, 1000, bc, 8), 38: diag_segment(3000, 36500, 38, 1000, bc, 8, spoil=2)})
    add("right_larger_wins", rd, [e0], fwd={37: diag_segment(3000, 36500, 37, 1000, bc, 8, spoil=2), 38: diag_segment(3000, 36500, 38, 1000, bc, 9)})
    add("right_score2_4", rd, [e0], fwd={37: diag_segment(3000, 36500, 37, 1000, bc, 4)})
    # (five seeds give one another four votes: find_location wants five, so the `score2 > 4` gate never decides alone)
    add("right_score2_5", rd, [e0], fwd={37: diag_segment(3000, 36500, 37, 1000, bc, 5)})
    add("right_score2_6", rd, [e0], fwd={37: diag_segment(3000, 36500, 37, 1000, bc, 6)})
    add("right_score2_25", rd, [e0], fwd={38: diag_segment(3000, 36500, 38, 1000, bc, 25)})
    add("right_no_location", rd, [e0], fwd={37: diag_segment(3000, 36500, 37, 1000, bc, 7), 38: garbage_segment(9, rng)})
    add("right_other_strand_db", rd, [e0], rev={37: diag_segment(3000, 36500, 37, 1000, bc, 8)})
    # the CLIPPED gate on the right, read side (5700 - qend) and reference side (G - send), at 2000 and 2001
    rd2 = two(53000, 3000, 57200, 2700)
    bc2 = bc_of(5700, 0)
    db2 = {59: diag_segment(3000, 57200, 59, 1000, bc2, 12)}
    for qend in (3699, 3700):
        add("right_gate_read_%d" % qend, rd2, [(0, qend, 0, 53000, 56000)], fwd=db2)
    for send in (G - 2001, G - 2000):
        add("right_gate_ref_%d" % (G - send), rd2, [(0, 3000, 0, 53000, send)], fwd=db2)
    # round 2: 2 000-base segments, stride 5
    add("right_attach_round2", rd, [e0], fwd={19: diag_segment(3000, 36500, 19, 2000, 5, 14)}, rnd=1)

    # left attach, reverse strand: the entries and the seeds are the reverse strand's, the read is handed over as its forward strand
    x = two(41000, 3000, 44500, 3000)
    # (the unmodified extension runs some 150 to 250 columns past the break, so the entry starts where the rescue result will end)
    e1 = (3200, 6000, 1, 44700, 47500)
    add("left_attach_R", comp(x), [e1], rev={42: diag_segment(0, 41000, 42, 1000, bc, 8, spoil=2), 43: diag_segment(0, 41000, 43, 1000, bc, 8)})
    add("left_tie_R", comp(x), [e1], rev={42: diag_segment(0, 41000, 42, 1000, bc, 8), 43: diag_segment(0, 41000, 43, 1000, bc, 8, spoil=2)})
    # the CLIPPED gate on the left: qoff and soff at 2000 and 2001 (entries that lie about where they are; the seeds do not)
    rd3 = two(500, 2500, 3300, 3000)
    bc3 = bc_of(5500, 0)
    db3 = {1: diag_segment(0, 500, 1, 1000, bc3, 10)}
    for qoff in (2000, 2001):
        add("left_gate_read_%d" % qoff, rd3, [(qoff, 5500, 0, 3300, 6300)], fwd=db3)
    for soff in (2000, 2001):
        add("left_gate_ref_%d" % soff, rd3, [(2500, 5500, 0, soff, 6300)], fwd=db3)

    # an ok rescue result that is not attached takes an id all the same: the second entry's right try finds the first stretch whole
    rd4 = two(33000, 4000, 41000, 3000)
    bc4 = bc_of(7000, 0)
    add("attached_then_unattached", rd4, [(0, 1500, 0, 33000, 34500), (4200, 7000, 0, 41200, 44000)], fwd={36: diag_segment(0, 33000, 36, 1000, bc4, 10)})
    # the first three entries are tried, the fourth is not
    four = [(0, 3000 - 10 * t, 0, 33000 - 200 * t, 36000 - 10 * t) for t in range(4)]
    add("fourth_not_tried", rd, four, fwd={37: diag_segment(3000, 36500, 37, 1000, bc, 8)})
    add("fourth_not_tried_out2", rd, four, fwd={37: diag_segment(3000, 36500, 37, 1000, bc, 8)}, num_output=2)
    # 0.9 of the read: at ceil(0.9 * qs) the tool returns before the searches, one below it rescues
    rd5 = two(20000, 19800, 40300, 2200)
    bc5 = bc_of(22000, 0)
    db5 = {41: diag_segment(19800, 40300, 41, 1000, bc5, 12)}
    for qend in (19800, 19799):
        add("full_edge_%d" % qend, rd5, [(0, qend, 0, 20000, 20000 + qend)], fwd=db5)
    # step 6: the attached rescue result covers 0.9 of the read, the array is cut to it
    rd6 = two(33000, 9200, 42500, 800)
    add("full_cut", rd6, [(9200, 10000, 0, 42500, 43300)], fwd={41: diag_segment(0, 33000, 41, 1000, bc_of(10000, 0), 10)})
    return cases


def case_input_words(c):
    """one case as the recorder reads it (int64 words around the read's letters) -> bytes"""
    w = lambda v: np.asarray(v, dtype="<i8").tobytes()
    out = [w([len(c["read"])]), c["read"].tobytes(), w([c["block_size"], c["bc"], c["num_output"], len(c["entries"])])]
    for e in c["entries"]:
        out.append(w(e))
    for db in (c["fwd"], c["rev"]):
        out.append(w([len(db)]))
        for seg in sorted(db):
            sc, loc, seed = db[seg]
            out.append(w([seg, sc] + list(loc) + list(seed)))
    return b"".join(out)


TOOL_RUNS = [(n, b) for n in (1, 2, 10) for b in (1, 10)]          # (-n, -b) of the recorded runs of the whole tool


def parse_tool_stream(t):
    """one run's record stream (tests/golden/ref_rescue_ref_main.cpp, tool mode) -> the calls in order: dict(read, read_len, block_size,
    bc, naln0, nres0, nres1, before [naln0][6], after [naln][9] (AFTER_FIELDS), results [nres1][10] (NEW_FIELDS), nbytes, crc, records)"""
    t = [int(x) for x in t]
    at, calls = 0, []
    while at < len(t):
        if t[at] == 1:
            _, read, read_len, bs, bc, naln0, nres0, naln1, nres1 = t[at: at + 9]
            at += 9
            c = dict(read=read, read_len=read_len, block_size=bs, bc=bc, naln0=naln0, nres0=nres0, nres1=nres1)
            c["before"] = [t[at + 6 * i: at + 6 * i + 6] for i in range(naln0)]
            at += 6 * naln0
            c["after"] = [t[at + 9 * i: at + 9 * i + 9] for i in range(naln1)]
            at += 9 * naln1
            c["results"] = [t[at + 10 * i: at + 10 * i + 10] for i in range(nres1)]
            at += 10 * nres1
            nev = t[at]
            ev = [t[at + 1 + 8 * i: at + 9 + 8 * i] for i in range(nev)]
            at += 1 + 8 * nev
            # finds: (side, read gate failed, reference gate failed, fill called, its score2, its return, the search's return);
            # extends (alns == NULL): (loc1, loc2, score, chain, return)
            c["finds"] = [tuple(e[1:8]) for e in ev if e[0] == 3]
            c["extends"] = [tuple(e[1:6]) for e in ev if e[0] == 4]
            assert len(c["finds"]) + len(c["extends"]) == nev
            calls.append(c)
        else:
            assert t[at] == 2 and calls and t[at + 1] == calls[-1]["read"] and "crc" not in calls[-1]
            calls[-1]["nbytes"], calls[-1]["crc"], calls[-1]["records"] = t[at + 2: at + 5]
            at += 5
    assert all("crc" in c for c in calls)
    return calls


_fx = None


def fixture():
    """ref_rescue.npz -> dict(cases: [case + recorded outcome], ref_letters, ref_codes, asserted).  A recorded outcome: after
    int64[naln, 9] (AFTER_FIELDS), nresults, new int64[k, 10] (NEW_FIELDS: the results the call added), printed [ids].
    tool_reads + tool {(-n, -b): calls}: the whole unmodified tool on chain_reads(), every call of the two functions (parse_tool_stream)"""
    global _fx
    if _fx is None:
        import ref_ext_cases as XC
        z = np.load(FIXTURE)
        base = RC.fixture()
        codes, let = XC.ref_codes(base["ref_fasta"].tobytes())
        meta = json.loads(str(z["cases"]))
        cases = []
        for i, m in enumerate(meta):
            c = dict(m)
            c["read"] = z["read_%d" % m["read"]]
            c["entries"] = [tuple(e) for e in m["entries"]]
            for k in ("fwd", "rev"):
                c[k] = {int(s): (v[0], v[1], v[2]) for s, v in m[k].items()}
            c["after"] = np.array(m["after"], dtype=np.int64).reshape(-1, len(AFTER_FIELDS))
            c["new"] = np.array(m["new"], dtype=np.int64).reshape(-1, len(NEW_FIELDS))
            cases.append(c)
        lens = z["tool_read_lens"]
        ends = np.cumsum(lens)
        tool_reads = [z["tool_reads"][e - n: e] for n, e in zip(lens, ends)]
        tool = {nb: parse_tool_stream(z["tool_n%d_b%d" % nb]) for nb in TOOL_RUNS}
        _fx = dict(cases=cases, ref_letters=let, ref_codes=codes, asserted=json.loads(str(z["asserted"])), tool_reads=tool_reads, tool=tool)
    return _fx


# ----------------------------------------------------------------------------- reads for the whole chain (seed -> extend -> rescue)
CHAIN_SEED = 20264


def _shared(r, src):
    ks = {bytes(src[i: i + 13]) for i in range(len(src) - 12)}
    return sum(bytes(r[i: i + 13]) in ks for i in range(len(r) - 12))


def chain_reads(codes):
    """codes: the reference as 0..3 -> [letters]: stretches of the reference at up to 15 % error (libsynth), put together on one strand,
    the whole read then on either strand"""
    rng = np.random.default_rng(CHAIN_SEED)
    G = len(codes)
    out = []
    made = [0]

    def fwd(a, n, err=0.15):
        """the reference's [a, a + n) as a read's stretch on the forward strand (libsynth picks the strand: a reverse draw is turned back)"""
        src = codes[a: a + n]
        made[0] += 1
        r = RC.one_read(src, made[0], n, err, CHAIN_SEED)
        back = (3 - r)[::-1]
        return back if _shared(back, src) > _shared(r, src) else r

    def add(parts):
        r = np.concatenate(parts)
        if rng.integers(0, 2):
            r = (3 - r)[::-1]
        out.append(RC.letters(r).copy())
    junk = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    for a, n in ((33000, 5000), (41000, 8000), (53000, 3500), (27000, 6500)):          # plain
        add([fwd(a, n)])
    for a, gap, err in ((30000, 2500, 0.15), (33000, 5000, 0.15), (28000, 9000, 0.12), (34000, 3000, 0.0), (41000, 2600, 0.05)):          # a deletion between two 4 kb halves
        add([fwd(a, 4000, err), fwd(a + 4000 + gap, 4000, err)])
    # the unmodified extension runs 150 to 450 columns past a break, and a rescue result is attached only within 200 of its owner: 300
    # random letters between the halves bring the two ends together
    for a, gap, err in ((30500, 3000, 0.0), (42000, 2500, 0.05), (28500, 4000, 0.10), (34500, 6000, 0.15), (21000, 3000, 0.02)):
        add([fwd(a, 4000, err), junk(300), fwd(a + 4000 + gap, 4000, err)])
    add([fwd(33000, 3500), junk(3000), fwd(36500, 3500)])          # 3 kb of random letters in the middle, at the head, at the tail
    add([junk(3000), fwd(42000, 5000)])
    add([fwd(28000, 5000), junk(3000)])
    mid = fwd(36000, 3000)
    add([fwd(33000, 3000), (3 - mid)[::-1], fwd(39000, 3000, 0.10)])          # an inverted middle
    add([fwd(22000, 4000), fwd(49500, 4000)])          # halves from two chromosomes
    add([fwd(55000, 4000, 0.10), fwd(27000, 3500, 0.10)])
    s0, ln, copies = 3000, 2000, (12500, 31000, 49000)          # the repeat planted by make_golden_ref_cand.py
    add([fwd(copies[1] - 4000, 4000), fwd(s0 + 200, 1700, 0.05), fwd(copies[1] + ln + 2500, 3000)])          # the missing part lies in a repeat copy
    add([fwd(200, 3000, 0.10), fwd(6000, 3500, 0.10)])          # near the reference's first base
    add([fwd(G - 9000, 3500, 0.10), fwd(G - 3200, 3000, 0.10)])          # and its last
    for a, n in ((45000, 1500), (36000, 3000), (58000, 1900)):          # under 4 kb
        add([fwd(a, n, 0.10)])
    # two 1 300-letter stretches at 22 % error between random letters: round 1 (stride by length, gate 6) finds nothing, round 2 (stride 5,
    # 2 000-base segments, gate 4) finds one of them and the rescue the other
    for a in (41000, 33500, 27500, 53000):
        add([junk(3000), fwd(a, 1300, 0.22), junk(3000), fwd(a + 3800, 1300, 0.22), junk(2500)])
    return out


# ----------------------------------------------------------------------------- mecat_amd/host/ref_results.cpp's ref_read_records through tests/ref_rescue_results_lib.cpp
_rl = None


def records_lib():
    global _rl
    if _rl is None:
        import ctypes as C
        import subprocess
        import tempfile
        so = os.path.join(tempfile.mkdtemp(prefix="refrescue_"), "libref_rescue_results.so")
        subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-I" + os.path.join(H.ROOT, "include"),
                        os.path.join(H.ROOT, "tests", "ref_rescue_results_lib.cpp"), "-o", so], check=True)
        L = C.CDLL(so)
        L.rrr_read_records.restype = C.c_int64
        L.rrr_read_records.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
        _rl = L
    return _rl


def lib_read_records(read_id, out_slots, first, first_offs, first_words, rescue, rescue_offs, rescue_words, reads_pac, reads_nplane, read_off, ref_pac):
    """ref_read_records for one read: first / rescue = the read's rows of the two fetches (REF_RESULT_DTYPE), *_offs = the rows' word
    offsets (one more than rows), *_words = the fetches' whole word arrays -> the bytes, or None when the function refuses"""
    import ctypes as C
    from mecat_amd import hip
    slots = np.ascontiguousarray(out_slots, dtype=np.int32)
    first = np.ascontiguousarray(first, dtype=hip.REF_RESULT_DTYPE)
    rescue = np.ascontiguousarray(rescue, dtype=hip.REF_RESULT_DTYPE)
    fo, ro = np.ascontiguousarray(first_offs, dtype=np.uint64), np.ascontiguousarray(rescue_offs, dtype=np.uint64)
    fw = np.ascontiguousarray(np.concatenate([first_words, [0]]), dtype=np.uint32)
    rw = np.ascontiguousarray(np.concatenate([rescue_words, [0]]), dtype=np.uint32)
    assert len(fo) == len(first) + 1 and len(ro) == len(rescue) + 1
    cap = 4 * 16 * (len(fw) + len(rw)) + 4096 * (len(slots) + 1)
    buf = C.create_string_buffer(cap)
    n = records_lib().rrr_read_records(read_id, slots.ctypes.data, len(slots), first.ctypes.data, fo.ctypes.data, fw.ctypes.data, len(first), rescue.ctypes.data,
                                       ro.ctypes.data, rw.ctypes.data, len(rescue), reads_pac.ctypes.data, reads_nplane.ctypes.data, int(read_off), ref_pac.ctypes.data,
                                       buf, cap)
    assert n != -2
    return None if n < 0 else buf.raw[:n]
