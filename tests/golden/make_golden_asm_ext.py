#!/usr/bin/env python3
"""Golden vectors for mhip_asm_extend: the extension loop of the UNMODIFIED pairwise_mapping of mecat2asmpw.c
(:723-841), column by column.  oracle/_ref/libref_asmpw_ext.so (oracle/ref_harness_asmpw_ext.c) is the reference file compiled as it
lies with a recording `string_check`: per candidate, in list order, the four aligned strings left_store1 / left_store2 / right_store1 /
right_store2 as the tool left them.  store1 is the row of the subject read (the indexed block, x: `align`'s query_seq, :757), store2
the row of the mapped read (y).  The restatement of the candidate stage (oracle/asmpw_oracle.c, fresh mode) runs beside it and names
the candidates, which become mhip_asm_job records by the formula of include/mecat_hip.h (x0 = loc1 - 1 - readstart; left from
(x0 + 12, loc2 + 12), right from (x0, loc2)); the strings' own bases are checked against the reads at those start points.
mecat2trimpw.c's loop is the same text (a whitespace-stripped diff of :729-859 shows nothing): one fixture serves both tools.
Build container only:
    python tests/golden/make_golden_asm_ext.py
Writes tests/golden/asm_ext.npz: per job the mhip_asm_job, per direction {cols, x bases, y bases, y-only, x-only} counted from the
strings and a SHA-256 over its columns (2-bit ops in extension order, 16 per little-endian uint32 word, as the header defines them),
the words themselves for every FULL_EVERY-th job and for the hand-built sets; the hand-built reads; the parameters of the others."""
import ctypes as C
import hashlib
import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import helpers as H  # noqa: E402

OUT = os.path.join(H.GOLDEN, "asm_ext.npz")
FULL_EVERY = 3
JOB_FIELDS = ("xid", "yid", "chain", "lx", "ly", "lnx", "lny", "rx", "ry", "rnx", "rny", "pad")
GOLDEN_GEN = dict(nreads=400, L=6000, err=0.02, genome=120000, seed=91, ont=0)       # == make_golden_asmpw.GEN

# kind "synth": H.synth_reads(**gen), reads numbered from 1; the block = reads block[0]..block[1], the mapped reads = `queries`
#               (first, last, step)
# kind "layout": mecat_amd.workload.asm_blocks_layout(dir, **layout) (Ns / IUPAC codes), block = its first block
# kind "hand": reads built below and stored in the file
SETS = [
    dict(name="golden_S1", kind="synth", gen=GOLDEN_GEN, block=(1, 200), queries=(1, 400, 9)),
    dict(name="golden_S2", kind="synth", gen=GOLDEN_GEN, block=(201, 400), queries=(201, 400, 9)),
    dict(name="err4", kind="synth", gen=dict(nreads=56, L=4000, err=0.04, genome=30000, seed=141, ont=0), block=(1, 28), queries=(1, 56, 1)),
    dict(name="err5", kind="synth", gen=dict(nreads=56, L=4000, err=0.05, genome=30000, seed=142, ont=0), block=(1, 28), queries=(1, 56, 1)),
    dict(name="err6", kind="synth", gen=dict(nreads=56, L=4000, err=0.06, genome=30000, seed=143, ont=0), block=(1, 28), queries=(1, 56, 1)),
    # 10 and 12 %: the error rate at which `align`'s limit (0.10 of the two blocks' bases, in O(ND) differences) does bind on these reads
    dict(name="err10", kind="synth", gen=dict(nreads=56, L=4000, err=0.10, genome=30000, seed=145, ont=0), block=(1, 28), queries=(1, 56, 1)),
    dict(name="err12", kind="synth", gen=dict(nreads=56, L=4000, err=0.12, genome=30000, seed=146, ont=0), block=(1, 28), queries=(1, 56, 1)),
    dict(name="with_n", kind="layout", layout=dict(nreads=120, L=4000, genome=40000, nblocks=2, seed=78, err=0.02, n_every=2, iupac=False),
         queries=(1, 120, 3)),
    dict(name="iupac", kind="layout", layout=dict(nreads=120, L=4000, genome=40000, nblocks=2, seed=79, err=0.02, n_every=0, iupac=True),
         queries=(2, 120, 3)),
    dict(name="ladder_r", kind="hand"),
    dict(name="ladder_l", kind="hand"),
    dict(name="edges", kind="hand"),
    dict(name="long", kind="hand"),
]
DEVICE_CANDIDATE_SETS = ("err4", "err5", "err6", "err10", "err12")      # every read is a query here: the GPU test rebuilds the jobs from mhip_asm_seed_reads

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    """the mapped strand as the tool makes it (:580-590): reversed, A / C / G / T complemented, every other character kept"""
    return s[::-1].translate(COMP)


def _noisy(rng, g, err):
    """a copy of g (uint8 codes) with err / 2 substitutions, err / 4 deletions, err / 4 insertions -> bytes over ACGT"""
    u = rng.random(len(g))
    out = []
    for c, r in zip(g.tolist(), u.tolist()):
        if r < err * 0.25:
            continue
        if r < err * 0.75:
            c = (c + 1 + int(rng.integers(0, 3))) % 4
        out.append(c)
        if r > 1.0 - err * 0.25:
            out.append(int(rng.integers(0, 4)))
    return bytes(b"ACGT"[c] for c in out)


# The tool takes the end of a block's last read from a table entry it never wrote (:640; zero on a fresh heap), which costs that read its
# candidates: the hand-built blocks end with a read nothing maps to.
DUMMY = b"ACGGTCATGCTTAGC" * 20


def _top_candidate(block, queries):
    """(x0, loc2, chain) of the first candidate of query 0 against a one-read block: where the tool puts its seed"""
    cands = _oracle_candidates(block + [DUMMY], 1, [(len(block) + 2, queries[0])])
    c = cands[0][0]
    return c.loc1 - 1 - c.readstart, c.loc2, c.chain


def _poison(y, n):
    """every 13th of the first n bases replaced: no 13-mer of that stretch is left for the tool to seed, and a block inside it carries
    2 / 13 of its length in O(ND) differences (a substitution costs two) besides the reads' own — under `align`'s limit, not by much"""
    b = bytearray(y)
    for i in range(6, n, 13):
        b[i] = b"CGTA"[b"ACGT".index(b[i])]
    return bytes(b)


def build_ladder(which):
    """One subject sequence X and one mapped read Y cut from one genome at 1 % error each (2 % between them).  The tool seeds Y's 13-mers
    at stride 10 and keeps one candidate per pair, at the first seeds of the overlap: the distance from Y's start to the seed moves in
    steps of ten and the left direction is short.  So the ladder is on the subject side — the block holds copies of X cut a bases in
    front of the seed / b bases behind it, a and b stepping one base at a time so that the bases available (a + 13, b + 13: both
    directions contain the seed) run through 585..615 and 1085..1115: a last block takes up to 600 bases, 500-base blocks above that,
    so both edges and the first block's tail cut lie inside — and for the left side Y2, a copy of Y whose first 1 300 bases cannot be
    seeded (_poison): its seed lies behind them and its left direction crosses them.  A read keeps at most 100 candidates, so the
    copies come as three blocks: "ladder_r", "ladder_l" and "edges" — copies with 0..13 bases on one side of the seed; Y2 and its reverse
    complement are the mapped reads of each.  For some copies the tool picks a seed ten or twenty bases further on, which leaves a few
    values of a range out (600 itself among them); a third mapped read, Y2 without its first 5 bases (right) / its first base (left),
    moves the stride-10 seeds against the copies and supplies them: main() asks for every value of 590..610 and 1090..1110 on both
    sides."""
    rng = np.random.default_rng(20261)
    g = rng.integers(0, 4, 6000, dtype=np.uint8)
    X, Y = _noisy(rng, g, 0.01), _noisy(rng, g, 0.01)
    Y2 = _poison(Y, 1300)
    x2, _, _ = _top_candidate([X], [Y2])
    assert 1250 < x2 < 1500, x2
    if which == "ladder_r":
        return [X[: x2 + 13 + base + j] for base in (572, 1072) for j in range(31)] + [DUMMY], [Y2, revcomp(Y2), Y2[5:]]
    if which == "ladder_l":
        return [X[x2 - (base + j): x2 + 13 + 1500] for base in (572, 1072) for j in range(31)] + [DUMMY], [Y2, revcomp(Y2), Y2[1:]]
    block = []
    for j in range(14):
        block.append(X[x2 - j: x2 + 13 + 1500])
        block.append(X[: x2 + 13 + j])
    return block + [DUMMY], [Y2, revcomp(Y2)]


def build_long():
    """one pair of 85 000-base reads (the tool's line buffers hold 100 000 characters): a direction of more than 40 000 columns"""
    rng = np.random.default_rng(20262)
    g = rng.integers(0, 4, 85000, dtype=np.uint8)
    return [_noisy(rng, g, 0.01), DUMMY], [_noisy(rng, g, 0.01)]


def set_reads(spec, stored=None):
    """-> (block reads [bytes], first read number of the block, mapped reads [(read number, bytes)]) of one set; `stored` = the loaded
    fixture (the hand-built sets are read from it; without it they are built)"""
    if spec["kind"] == "synth":
        g = spec["gen"]
        codes, lens = H.synth_reads(g["nreads"], g["L"], g["err"], g["genome"], g["seed"], g["ont"])
        starts = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
        lut = np.frombuffer(b"ACGT", dtype=np.uint8)
        read = lambda rid: lut[codes[starts[rid - 1]: starts[rid]]].tobytes()      # noqa: E731
        b, e = spec["block"]
        q0, q1, qs = spec["queries"]
        return [read(r) for r in range(b, e + 1)], b, [(r, read(r)) for r in range(q0, q1 + 1, qs)]
    if spec["kind"] == "layout":
        sys.path.insert(0, H.ROOT)
        from mecat_amd import workload as W
        with tempfile.TemporaryDirectory() as d:
            lo = spec["layout"]
            blocks, _ = W.asm_blocks_layout(d, lo["nreads"], lo["L"], lo["genome"], lo["nblocks"], lo["seed"], err=lo["err"], n_every=lo["n_every"],
                                            iupac=lo["iupac"])
            reads = {}
            for k in range(len(blocks)):
                lines = open(os.path.join(d, "%06d.fasta" % (k + 1)), "rb").read().split(b"\n")
                for h, s in zip(lines[0::2], lines[1::2]):
                    reads[int(h[1:])] = s.upper()             # the tool upper-cases what it reads (:398, 992)
        b, e = blocks[0]
        q0, q1, qs = spec["queries"]
        return [reads[r] for r in range(b, e + 1)], b, [(r, reads[r]) for r in range(q0, q1 + 1, qs)]
    name = spec["name"]
    if stored is None:
        block, queries = build_long() if name == "long" else build_ladder(name)
    else:
        def cut(key):
            t, ln = stored["hand_%s_%s" % (name, key)].tobytes(), stored["hand_%s_%s_lens" % (name, key)]
            at = np.concatenate([[0], np.cumsum(ln)])
            return [t[at[i]: at[i + 1]] for i in range(len(ln))]
        block, queries = cut("block"), cut("queries")
    return block, 1, [(len(block) + 1 + i, q) for i, q in enumerate(queries)]


class _Cand(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("loc1", "loc2", "left1", "left2", "right1", "right2", "score", "num1", "num2", "readno", "readstart")] + [("chain", C.c_char)]


def _block_text(block):
    st, off = [], 0
    for s in block:
        st.append(off)
        off += len(s) + 1
    return b"".join(s + b"\0" for s in block), np.array(st, dtype=np.int32), np.array([len(s) for s in block], dtype=np.int32)


def _oracle_candidates(block, first_no, queries):
    """oracle/asmpw_oracle.c, fresh mode: the candidates of every mapped read in list order -> [[_Cand copies]]"""
    H.orc()
    O = C.CDLL(os.path.join(H.ROOT, "oracle", "liboracle.so"))
    O.asm_block_new.restype = C.c_void_p
    O.asm_block_new.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    O.asm_candidates.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    O.asm_block_fresh.argtypes = [C.c_void_p, C.c_int]
    O.asm_block_free.argtypes = [C.c_void_p]
    text, st, _ = _block_text(block)
    tbuf = C.create_string_buffer(text, len(text))
    B = O.asm_block_new(tbuf, len(text), st.ctypes.data, len(block), first_no)
    O.asm_block_fresh(B, 1)
    out = (_Cand * 100)()
    res = []
    for name, q in queries:
        n = O.asm_candidates(B, q, len(q), name, out)
        res.append([_Cand.from_buffer_copy(out[i]) for i in range(n)])
    O.asm_block_free(B)
    return res


def job_of(c, yid):
    """mhip_asm_job from a candidate (include/mecat_hip.h; mecat_amd/asmpw/asmpw_main.cpp does the same)"""
    x0 = c.loc1 - 1 - c.readstart
    chain = 0 if c.chain == b"F" else 1
    return (c.readno, yid, chain, x0 + 12, c.loc2 + 12, c.left1, c.left2, x0, c.loc2, c.right1, c.right2, 0)


def pack_ops(s1, s2):
    """the columns of one direction as 2-bit ops, 16 per uint32 from the least significant bits: 0 both bases, 1 y base only (a gap in
    store1, the subject's row), 2 x base only"""
    a, b = np.frombuffer(s1, dtype=np.uint8), np.frombuffer(s2, dtype=np.uint8)
    ops = np.where(a == 45, 1, np.where(b == 45, 2, 0)).astype(np.uint32)
    ops = np.concatenate([ops, np.zeros(-len(ops) % 16, dtype=np.uint32)]).reshape(-1, 16)
    return (ops << (2 * np.arange(16, dtype=np.uint32))[None, :]).sum(axis=1, dtype=np.uint64).astype("<u4")


def run_set(spec):
    """the reference's strings for every candidate of every mapped read of the set -> per job (job tuple, [left, right] x (s1, s2))"""
    block, first_no, queries = set_reads(spec)
    R = C.CDLL(os.path.join(H.ROOT, "oracle", "_ref", "libref_asmpw_ext.so"))
    R.refasme_setup.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    R.refasme_extend.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    text, st, ln = _block_text(block)
    tbuf = C.create_string_buffer(text, len(text))
    R.refasme_setup(tbuf, len(text), st.ctypes.data, ln.ctypes.data, len(block), first_no)
    cands = _oracle_candidates(block, first_no, queries)
    rec = np.zeros(96_000_000, dtype=np.uint8)
    jobs = []
    for yid, ((name, q), cl) in enumerate(zip(queries, cands)):
        assert len(q) < 99_999
        used = C.c_long()
        ncalls = R.refasme_extend(C.create_string_buffer(q), name, rec.ctypes.data, len(rec), C.byref(used))
        assert ncalls == len(cl), (spec["name"], name, ncalls, len(cl))       # one string_check call per candidate
        raw, at = rec[: used.value].tobytes(), 0
        strands = (q, revcomp(q))
        for c in cl:
            lens = np.frombuffer(raw[at: at + 16], dtype=np.int32)
            at += 16
            s = []
            for n in lens:
                s.append(raw[at: at + n])
                at += n
            assert len(s[0]) == len(s[1]) and len(s[2]) == len(s[3])
            jb = job_of(c, yid)
            # the strings' bases are the reads' bases from the job's start points on: this candidate IS that call
            x, y = block[jb[0]], strands[jb[2]]
            xl, yl, xr, yr = (t.replace(b"-", b"") for t in s)
            assert xl == x[max(0, jb[3] - len(xl) + 1): jb[3] + 1][::-1] and yl == y[max(0, jb[4] - len(yl) + 1): jb[4] + 1][::-1], (spec["name"], name, jb)
            assert xr == x[jb[7]: jb[7] + len(xr)] and yr == y[jb[8]: jb[8] + len(yr)], (spec["name"], name, jb)
            jobs.append((jb, ((s[0], s[1]), (s[2], s[3]))))
        assert at == len(raw)
    return jobs


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates and order: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)


def main(out=OUT):
    jobs, dirs, shas, full_dirs, full_words, ranges = [], [], [], [], [], {}
    arrays = {}
    cov = dict(dirs=0, early=[0, 0], zero=0, strands=set(), ncol=0, last_block=0, mod16=set(), long=0, edge=0)
    ladder = dict(left=set(), right=set())
    for spec in SETS:
        res = run_set(spec)
        first = len(jobs)
        for jb, pairs in res:
            ji = len(jobs)
            jobs.append(jb)
            cov["strands"].add(jb[2])
            for d, (s1, s2) in enumerate(pairs):
                a, b = np.frombuffer(s1, dtype=np.uint8), np.frombuffer(s2, dtype=np.uint8)
                both = (a != 45) & (b != 45)
                assert np.array_equal(a[both], b[both]), (spec["name"], jb, d)         # O(ND): no mismatch columns
                assert not ((a == 45) & (b == 45)).any()
                cols, xb, yb = len(a), int((a != 45).sum()), int((b != 45).sum())
                dirs.append((cols, xb, yb, cols - xb, cols - yb))
                w = pack_ops(s1, s2)
                shas.append(np.frombuffer(hashlib.sha256(w.tobytes()).digest(), dtype=np.uint8))
                if spec["kind"] == "hand" or ji % FULL_EVERY == 0:
                    full_dirs.append(2 * ji + d)
                    full_words.append(w)
                # coverage, from the strings and the candidate's sizes alone
                nx, ny = (jb[5], jb[6]) if d == 0 else (jb[9], jb[10])
                cov["dirs"] += 1
                # a last block has at most 600 bases a side and `align` gives up beyond 0.10 * 1200 = 120 differences, so a direction that
                # ran to its end leaves at most 120 bases of the longer side: more on BOTH sides = a block failed or was dropped
                cov["early"][d] += min(nx - xb, ny - yb) > 120
                cov["zero"] += cols == 0
                cov["ncol"] += bool((~np.isin(a, list(b"ACGT-")) | ~np.isin(b, list(b"ACGT-"))).any())
                cov["last_block"] += 500 < min(nx, ny) <= 600            # the only block of such a direction is its last one
                cov["mod16"].add(cols % 16)
                cov["long"] += cols > 40000
                cov["edge"] += min(nx, ny) <= 13
                if (spec["name"], d) in (("ladder_l", 0), ("ladder_r", 1)):
                    ladder["left" if d == 0 else "right"].add(min(nx, ny))
        ranges[spec["name"]] = (first, len(jobs))
        print("%-10s %5d jobs" % (spec["name"], len(jobs) - first), file=sys.stderr)
        if spec["kind"] == "hand":
            block, _, queries = set_reads(spec)
            for key, lst in (("block", block), ("queries", [q for _, q in queries])):
                arrays["hand_%s_%s" % (spec["name"], key)] = np.frombuffer(b"".join(lst), dtype=np.uint8)
                arrays["hand_%s_%s_lens" % (spec["name"], key)] = np.array([len(s) for s in lst], dtype=np.int64)
    print(json.dumps({k: (sorted(v) if isinstance(v, set) else v) for k, v in cov.items()}), file=sys.stderr)
    print("ladder left", sorted(ladder["left"]), "right", sorted(ladder["right"]), file=sys.stderr)
    assert cov["dirs"] >= 3000
    assert sum(cov["early"]) >= 200 and min(cov["early"]) > 0
    assert cov["zero"] >= 20
    assert cov["strands"] == {0, 1}
    assert cov["ncol"] >= 50
    assert cov["last_block"] >= 30
    assert {0, 1, 15} <= cov["mod16"]
    assert cov["long"] >= 1 and cov["edge"] >= 1
    for side in ("left", "right"):
        for lo in (590, 1090):
            assert set(range(lo, lo + 21)) <= ladder[side], (side, lo, sorted(set(range(lo, lo + 21)) - ladder[side]))
    arrays["meta"] = np.frombuffer(json.dumps(dict(sets=SETS, ranges=ranges, job_fields=JOB_FIELDS, full_every=FULL_EVERY), sort_keys=True).encode(), dtype=np.uint8)
    arrays["jobs"] = np.array(jobs, dtype=np.int32)
    arrays["dirs"] = np.array(dirs, dtype=np.int32)
    arrays["sha256"] = np.array(shas, dtype=np.uint8)
    arrays["full_dirs"] = np.array(full_dirs, dtype=np.int64)
    arrays["full_offs"] = np.concatenate([[0], np.cumsum([len(w) for w in full_words])]).astype(np.int64)
    arrays["full_words"] = np.concatenate(full_words).astype("<u4")
    write_npz(out, arrays)
    print("%s: %d jobs, %d bytes" % (out, len(jobs), os.path.getsize(out)), file=sys.stderr)
    assert os.path.getsize(out) < 1_000_000


if __name__ == "__main__":
    main()
