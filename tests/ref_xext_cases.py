"""Inputs and fixture access shared by the tests of mecat2ref's extension stage in nanopore mode (tests/golden/ref_xext.npz, made by
tests/golden/make_golden_ref_xext.py from the unmodified reference).  Two input sets: set 0 is ref_cand.npz's reference and reads with
its recorded `-x 1` lists and make_golden_ref_ext.hand_made's candidates; set 1 is second_set() below, a small reference of random
flanks around homopolymer and short-period tandem stretches with reads across them (the blocks whose window outgrows the ring block),
and crafted pairs in which every fourth base is substituted from a point on (no run of four matches: trim_mismatch_end fails)."""
import ctypes as C
import json
import os

import numpy as np

import helpers as H
import ref_cand_cases as RC
import ref_ext_cases as XC
import ref_ext_ref as X
import ref_rescue_cases as SC

FIXTURE = os.path.join(H.GOLDEN, "ref_xext.npz")
CAND_FIELDS = ("read", "chain", "loc1", "loc2", "score")
RES_FIELDS = ("ok", "qb", "qe", "qs", "sb", "se", "cols", "matches")
DIR_FIELDS = ("cols", "blocks", "sized_last", "xdrop_end", "failed_trim")
SRC_HAND, SRC_R1, SRC_R2, SRC_LOWC, SRC_CRAFT = 0, 1, 2, 3, 4
MIN_SPAN = 1000          # extend_candidate's min_aln_size: XdropAligner::go compares the QUERY SPAN with it
TOOL_RUNS = [(10, 10), (2, 1)]          # (-n, -b) of the recorded `-x 1` runs of the whole tool
SEED = 20266


def mutated(g, rng, err):
    """a forward copy of g with substitutions, insertions and deletions at rate err -> codes"""
    out = []
    for b in g:
        u = rng.random()
        if u < err / 3:
            continue
        if u < 2 * err / 3:
            out.append(int(rng.integers(0, 4)))
        out.append(int(b) if u >= err else int((b + 1 + rng.integers(0, 3)) % 4))
    return np.array(out, dtype=np.uint8)


def every_fourth(codes, start, step):
    """codes with every fourth base substituted from index `start` on, going right (step 1) or left (step -1)"""
    r = np.array(codes, dtype=np.uint8)
    idx = np.arange(start, len(r) if step > 0 else -1, 4 * step)
    r[idx] = (r[idx] + 1) % 4
    return r


CRAFT_LEN, CRAFT_START = 3000, 1400          # the crafted region's length, the start point inside it


def second_set():
    """-> (reference FASTA text, reads as letters, cands int64[m, 5], source int[m]): everything derived from SEED"""
    rng = np.random.default_rng(SEED)
    rand = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    tand = lambda unit, n: np.tile(np.array(unit, dtype=np.uint8), n // len(unit) + 1)[:n]
    parts = [rand(1200), tand([0], 500), rand(700), tand([0, 1], 600), rand(700), tand([0, 1, 2], 600), rand(600), tand([3, 3, 1, 0, 2], 500), rand(700),
             tand([2], 800), rand(1200)]
    low_end = sum(len(p) for p in parts)
    craft0 = low_end
    parts += [rand(CRAFT_LEN), rand(300)]
    g = np.concatenate(parts)
    G = len(g)
    text = RC.fasta_bytes([b"lowc"], [RC.letters(g)], width=60)
    reads, cands, source = [], [], []

    def add(r, chain, starts, src):
        r = RC.letters(r).copy()
        if chain:          # the stored read is the other strand: all of it reversed, upper-case letters complemented
            r = X.strand_letters(r, 1).copy()
        rid = len(reads)
        reads.append(r)
        for qs, rs in starts:          # (read_start on the mapped strand, ref_start)
            if 0 <= qs < len(r) and 0 <= rs < G:
                cands.append((rid, chain, rs + 1, qs, 7))
                source.append(src)
    # reads across the low-complexity stretches, start points in and around them, a little off the diagonal
    for k in range(24):
        a = int(rng.integers(0, low_end - 3500))
        b = a + int(rng.integers(2500, 3500))
        r = mutated(g[a:b], rng, (0.12, 0.05, 0.2)[k % 3])
        starts = []
        for _ in range(3):
            qs = int(rng.integers(0, len(r)))
            starts.append((qs, min(max(a + int(qs * (b - a) / len(r)) + int(rng.integers(-20, 20)), 0), G - 1)))
        add(r, k % 2, starts, SRC_LOWC)
    # crafted pairs: the region exactly, then every fourth base substituted from `p` bases behind the start point on (to the right),
    # or from `p` bases in front of it on (to the left)
    reg = g[craft0: craft0 + CRAFT_LEN]
    for chain in (0, 1):
        for p in (0, 300):
            add(every_fourth(reg, CRAFT_START + p, 1), chain, [(CRAFT_START, craft0 + CRAFT_START)], SRC_CRAFT)
            add(every_fourth(reg, CRAFT_START - 1 - p, -1), chain, [(CRAFT_START, craft0 + CRAFT_START)], SRC_CRAFT)
    return text, reads, np.array(cands, dtype=np.int64), np.array(source, dtype=np.int8)


def extra_chain_reads(codes):
    """reads for the rescue chain beside tests/ref_rescue_cases.py's chain_reads.  Under X-drop those attach nothing: with reward 1 and
    penalties of 1 an extension drifts on through unrelated sequence, hundreds of bases past a break, and a rescue result is attached
    only within 200 of its owner.  Here a homopolymer stretch stands between two halves from places 2.5 to 6 kb apart: against the
    reference it loses about half a point per base, so both extensions stop inside it.  -> [letters]"""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for a, gap, err, base, strand in ((30500, 3000, 0.05, 0, 0), (42000, 2500, 0.10, 3, 1), (28500, 4000, 0.12, 1, 0), (34500, 6000, 0.08, 2, 1)):
        r = np.concatenate([mutated(codes[a: a + 4000], rng, err), np.full(150, base, dtype=np.uint8), mutated(codes[a + 4000 + gap: a + 8000 + gap], rng, err)])
        if strand:
            r = (3 - r)[::-1]
        out.append(RC.letters(r).copy())
    return out


def chain_reads():
    """the rescue chain's reads: ref_rescue.npz's (== chain_reads() of tests/ref_rescue_cases.py) and the fixture's extra ones"""
    return list(SC.fixture()["tool_reads"]) + list(fixture()["tool_extra_reads"])


# ----------------------------------------------------------------------------- the expected value for fresh cases: liboracle's orc_xdrop_go
_xa = None


def xgo(ref_codes, read_letters, chain, loc1, loc2):
    """extend_candidate with an XdropAligner for one candidate, by oracle/liboracle.so's orc_xdrop_go on extract_sequences' window
    (tests/ref_ext_ref.py: window, strand_letters) -> dict over RES_FIELDS"""
    global _xa
    O = H.orc()
    if _xa is None:
        _xa = O.orc_xaligner_new()
    q = np.ascontiguousarray(X.ENCODE[X.strand_letters(read_letters, chain)], dtype=np.int8)
    ref_start, read_start, left, right = X.window(len(ref_codes), len(q), loc1, loc2)
    t = np.ascontiguousarray(ref_codes[ref_start - left: ref_start + right], dtype=np.int8)
    o = H.OrcAlnResult()
    O.orc_xdrop_go(_xa, q.ctypes.data, read_start, len(q), t.ctypes.data, left, len(t), MIN_SPAN, C.byref(o))
    return dict(ok=int(o.ok), qb=o.query_start, qe=o.query_end, qs=len(q), sb=ref_start - left + o.target_start, se=ref_start - left + o.target_end,
                cols=o.columns, matches=o.matches)


def columns_of(qmap, smap):
    """the two strings -> the 2-bit columns (0 = both bases, equal or not; 1 = target base only; 2 = query base only), 16 per uint32"""
    a, b = np.frombuffer(qmap, dtype=np.uint8), np.frombuffer(smap, dtype=np.uint8)
    assert len(a) == len(b) and not ((a == 45) & (b == 45)).any()
    op = np.where(a == 45, 1, np.where(b == 45, 2, 0)).astype(np.uint64)
    op = np.concatenate([op, np.zeros(-len(op) % 16, dtype=np.uint64)]).reshape(-1, 16)
    return (op << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


_fx = None


def fixture():
    """ref_xext.npz -> dict: cands int64[n, 5], set [n] (0 / 1), source [n] (SRC_*), res int64[n, 8] (RES_FIELDS), dirs [n, 2, 5]
    (DIR_FIELDS; left, right as align_ex leaves them), crc uint32[n, 2] (ok results), stored / stored_offs / stored_words, asserted;
    sets = [dict(read_list, ref_fasta, ref_codes, ref_letters)] for set 0 and 1; tool = {(-n, -b): calls} of the `-x 1` runs of the whole
    tool on tests/ref_rescue_cases.py's chain reads (parse_tool_stream)"""
    global _fx
    if _fx is None:
        z = np.load(FIXTURE)
        fx = {k: z[k] for k in z.files if not k.startswith("tool_x_")}
        fx["asserted"] = json.loads(str(z["asserted"]))
        base = RC.fixture()
        text, reads, cands, source = second_set()
        fx["sets"] = []
        for fasta, rl in ((base["ref_fasta"].tobytes(), base["read_list"]), (text, reads)):
            codes, let = XC.ref_codes(fasta)
            fx["sets"].append(dict(read_list=rl, ref_fasta=fasta, ref_codes=codes, ref_letters=let))
        ends = np.cumsum(z["tool_x_read_lens"])
        fx["tool_extra_reads"] = [z["tool_x_reads"][e - n: e] for n, e in zip(z["tool_x_read_lens"], ends)]
        fx["tool"] = {nb: SC.parse_tool_stream(z["tool_x_n%d_b%d" % nb]) for nb in TOOL_RUNS}
        _fx = fx
    return _fx
