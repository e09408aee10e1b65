"""The corrected reads, restated literally (mecat2cns/mecat_correction.cpp): meap_consensus_one_segment's target (:88-107), the size filter
of consensus_worker (:233) and output_cns_result (:155-188), from a table, ident bytes, a plan and the windows' consensus strings.  Also
here, for test_cns_reads_ref_cpu.py, test_gpu_cns_reads.py and golden/make_golden_cns_reads.py: cases of one template each (letters,
alignments (qaln, saln, soff, send), tech, min_cov, min_size, read_id) — hand-written edges, seeded random templates from cns_poa_cases'
generator, and generated long cases around the block rule —, the packed case file the reference driver reads, the fixture's arrays, the
whole back end on the host (cns_table_ref, cns_plan_ref, the piece cursor and libcns_poa_host.so's window routine, each pinned to the
compiled reference by its own test) as the restatement's inputs, and the exported split function through ctypes."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import numpy as np

import cns_pieces_ref as Q
import cns_plan_ref as PR
import cns_poa_cases as P
import cns_table_ref as T

ROOT = P.ROOT
GOLDEN = P.GOLDEN
FIXTURE = os.path.join(GOLDEN, "cns_reads.npz")
MAGIC = 0x52454131
FMAT = 1
MAX_SEQ, OVLP = 60000, 10000          # output_cns_result's MaxSeqSize and OvlpSize
BLK = MAX_SEQ - OVLP - 1000           # BlkSize
READ_DTYPE = np.dtype([("read_id", np.int32), ("range_beg", np.int32), ("range_end", np.int32), ("size", np.int32), ("seq_begin", np.int64),
                       ("template_index", np.int32), ("segment", np.int32)])
FIXTURE_SEED, FRESH_SEED, N_RANDOM = 20271, 20272, 200
LONG_SIZES = (59999, 60000, 60001, 99000, 99001)


# ---- the restatement

def segment_target(base, ident, beg, end, windows, strings):
    """meap_consensus_one_segment (:88-107) on positions [beg, end).  base / ident: the template's table bases and ident bytes; windows:
    the segment's listed (sb, se) in ascending order, strings: their `cns`.  -> bytes"""
    listed = {int(w[0]): i for i, w in enumerate(windows)}
    target = bytearray()
    n = end - beg
    i = 0
    while i < n and not (ident[beg + i] & FMAT):                   # :91
        i += 1
    while i < n:                                                   # :92
        target.append(int(base[beg + i]))                          # :94
        j = i + 1
        while j < n and not (ident[beg + j] & FMAT):               # :96
            j += 1
        if i + beg in listed:                                      # need_refinement (:98-101): what the plan lists
            cns = strings[listed[i + beg]]
            if len(cns) > 2:                                       # :104
                target += cns[1: len(cns) - 1]
        i = j
    return bytes(target)


def split(size, beg, end):
    """output_cns_result (:155-188) -> list of (L, R, range0, range1)"""
    if size <= MAX_SEQ:                                            # :168
        return [(0, size, beg, end)]
    out = []
    cutoff = size - OVLP - 1000                                    # :174
    L = 0
    while True:                                                    # :176-186
        R = L + BLK
        if R >= cutoff:
            R = size
        out.append((L, R, L + beg, R + beg if (R < size and R + beg < end) else end))
        L = R - OVLP
        if not R < size:
            return out


def reads_of(base, ident, segs, wins, strings, min_size, read_id, template_index=0, seg_base=0, win_base=0):
    """consensus_worker's output for one template's segments (records of cns_plan_ref / mecat_amd.hip: beg, end, win_begin, win_end) ->
    (list of (read_id, range0, range1, size, L, template_index, segment, target number), list of the kept targets)"""
    recs, targets = [], []
    for k, s in enumerate(segs):
        w0, w1 = int(s["win_begin"]) - win_base, int(s["win_end"]) - win_base
        target = segment_target(base, ident, int(s["beg"]), int(s["end"]), [(int(w["sb"]), int(w["se"])) for w in wins[w0: w1]], strings[w0: w1])
        if len(target) >= min_size:                                # :233
            for L, R, r0, r1 in split(len(target), int(s["beg"]), int(s["end"])):
                recs.append((read_id, r0, r1, R - L, L, template_index, seg_base + k, len(targets)))
            targets.append(target)
    return recs, targets


def as_arrays(recs, targets):
    """-> (reads [READ_DTYPE] with seq_begin into the targets stored once behind one another, seq uint8)"""
    start = np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.int64)
    out = np.zeros(len(recs), READ_DTYPE)
    for i, (rid, r0, r1, size, L, t, sg, tn) in enumerate(recs):
        out[i] = (rid, r0, r1, size, start[tn] + L, t, sg)
    return out, np.frombuffer(b"".join(targets), dtype=np.uint8)


def format_reads(reads, seq):
    """reads_correction_can.cpp:44-46"""
    seq = np.asarray(seq, np.uint8).tobytes()
    return b"".join(b">%d_%d_%d_%d\n%s\n" % (r["read_id"], r["range_beg"], r["range_end"], r["size"], seq[r["seq_begin"]: r["seq_begin"] + r["size"]]) for r in reads)


def results_of(reads, seq):
    """records with their letters, the form the reference driver's output is read into: list of (id, range0, range1, seq bytes)"""
    seq = np.asarray(seq, np.uint8).tobytes()
    return [(int(r["read_id"]), int(r["range_beg"]), int(r["range_end"]), seq[int(r["seq_begin"]): int(r["seq_begin"]) + int(r["size"])]) for r in reads]


# ---- the back end on the host, in front of the restatement

def host_back_end(c):
    """one case -> dict(table, ident, plan, strings, reads, seq): the table (cns_table_ref), the plan (cns_plan_ref), the windows' strings
    (the piece cursor + libcns_poa_host.so) and the restatement over them"""
    table, ident = T.build_table([(q, s, soff) for q, s, soff, _ in c["alns"]], c["tmpl"])
    plan = PR.plan([(table, ident, [(a[2], a[3]) for a in c["alns"]])], c["tech"], c["min_cov"], c["min_size"])
    wins = plan["windows"]
    strings = []
    if len(wins):
        strings, _ = P.host_run(P.case(c["alns"], [(int(w["sb"]), int(w["se"]), int(w["cov"])) for w in wins]))
    recs, targets = reads_of(table["base"].tolist(), ident.tolist(), plan["segments"], wins, strings, c["min_size"], c["read_id"])
    reads, seq = as_arrays(recs, targets)
    return dict(table=table, ident=ident, plan=plan, strings=strings, reads=reads, seq=seq)


# ---- cases

def case(tmpl, alns, tech, min_cov, min_size, read_id=7, long=None):
    return dict(tmpl=bytes(tmpl), alns=list(alns), tech=int(tech), min_cov=int(min_cov), min_size=int(min_size), read_id=int(read_id), long=long)


def _letters(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def _aln(tmpl, soff, end, ins=(), dele=()):
    """an alignment that copies tmpl[soff: end] with insertions {position: letters} in front of a position and deleted positions"""
    ins, dele = dict(ins), set(dele)
    q, s = bytearray(), bytearray()
    for p in range(soff, end):
        for ch in ins.get(p, b"") if p > soff else b"":
            q.append(ch); s.append(Q.GAP)
        s.append(tmpl[p])
        q.append(Q.GAP if p in dele else tmpl[p])
    return bytes(q), bytes(s), soff, end


def hand_cases():
    rng = np.random.default_rng(5)
    t = _letters(rng, 300)
    whole = lambda **kw: _aln(t, 0, 300, **kw)
    out = [
        case(t, [whole()] * 3, 1, 2, 40),                                                      # every position an anchor, no window
        case(t, [whole(ins={50: b"T", 64: b"GG", 65: b"A", 66: b"C"})] * 3, 1, 2, 40),          # windows at 63, 64, 65
        case(t, [whole(dele=range(0, 70))] * 3 + [whole()], 1, 2, 40),                         # no anchor in the first 70 positions
        case(t, [whole(dele=range(0, 300))] * 3, 1, 2, 40),                                    # no anchor at all: no read
        case(t, [whole(dele=range(290, 300))] * 3, 1, 2, 40),                                  # a last window that ends at the segment's end
        case(t, [whole(dele=range(60, 200), ins={210: b"ACGT" * 5})] * 2 + [whole()] * 2, 1, 2, 40),   # a window over three steps; two outvoted
        case(t, [whole(ins={100: b"T" * 150})] * 3, 1, 3, 40),                                  # a long window string
        case(t, [_aln(t, 0, 120)] * 3 + [_aln(t, 150, 300)] * 3, 0, 2, 50),                      # two segments of one template
        case(t, [_aln(t, 0, 120)] * 3 + [_aln(t, 150, 300)] * 3, 0, 2, 126),                     # ... the first too short for min_size
        case(t[:100], [_aln(t, 10, 90)] * 3, 1, 3, 80),                                        # a target of exactly min_size letters
        case(t[:100], [_aln(t, 10, 90)] * 3, 1, 3, 81),                                        # ... and of min_size - 1
        case(t[:100], [_aln(t, 10, 90, dele=(40,))] * 3, 1, 3, 80),                            # a run long enough, its target too short
        case(t, [whole()] * 2, 1, 3, 40),                                                      # too little coverage
        case(t, [], 0, 2, 40),                                                                 # nothing accepted
        case(t, [whole(ins={30: b"A"}), whole(ins={30: b"C"}), whole(dele=(31, 32)), whole(ins={200: b"GT"}), whole()], 0, 2, 40),
    ]
    return out


def template_of(alns, L):
    """the template an agreeing case's alignments copy (positions no alignment covers: A)"""
    t = bytearray(b"A" * L)
    for _, s, soff, _ in alns:
        p = soff
        for ch in s:
            if ch != Q.GAP:
                t[p] = ch
                p += 1
    return bytes(t)


def random_cases(seed, count):
    """templates of 150 .. 700 positions with 4 .. 12 alignments from cns_poa_cases.agreeing_case, min_size 40 .. 200, min_cov 2 .. 4; two
    in three have every alignment over the whole template, so that most give a read"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        L = int(rng.integers(150, 701))
        c = P.agreeing_case(rng, L, int(rng.integers(4, 13)), float(rng.choice([0.02, 0.05, 0.12])), whole=i % 3 != 2)
        out.append(case(template_of(c["alns"], L), c["alns"], int(rng.integers(0, 2)), int(rng.integers(2, 5)), int(rng.integers(40, 201)), read_id=1000 + i))
    return out


def long_case(kind, n, seed):
    """generated cases around the block rule: three identical alignments over positions [7, 7 + n) of a template of n + 12 letters.
    kind 0: every column a match, so the target is the n positions themselves (size n = end - beg); kind 1: an insertion of eight letters
    in front of every 32nd position (a target longer than end - beg); kind 2: every 16th position deleted (shorter)"""
    rng = np.random.default_rng(seed)
    tmpl = _letters(rng, n + 12)
    if kind == 0:
        a = (tmpl[7: 7 + n], tmpl[7: 7 + n], 7, 7 + n)
    elif kind == 1:
        a = _aln(tmpl, 7, 7 + n, ins={p: b"ACGTTGCA" for p in range(20, 7 + n, 32)})
    else:
        a = _aln(tmpl, 7, 7 + n, dele=range(20, 7 + n - 8, 16))
    return case(tmpl, [a] * 3, 1, 3, 5000, read_id=31 + kind, long=(int(kind), int(n), int(seed)))


def long_cases():
    return [long_case(0, n, 100 + i) for i, n in enumerate(LONG_SIZES)] + [long_case(1, 48500, 200), long_case(2, 70000, 201)]


def fixture_cases():
    return hand_cases() + random_cases(FIXTURE_SEED, N_RANDOM) + long_cases()


# ---- the reference driver

def write_cases(path, cases):
    """the packed case file: int32 MAGIC, cases; per case tech, min_cov, min_size, read_id, the template's length and letters, the number of
    alignments, per alignment soff, send, len and the bytes of qaln and saln"""
    with open(path, "wb") as f:
        f.write(struct.pack("<2i", MAGIC, len(cases)))
        for c in cases:
            f.write(struct.pack("<5i", c["tech"], c["min_cov"], c["min_size"], c["read_id"], len(c["tmpl"])) + c["tmpl"])
            f.write(struct.pack("<i", len(c["alns"])))
            for q, s, soff, send in c["alns"]:
                f.write(struct.pack("<3i", soff, send, len(q)) + bytes(q) + bytes(s))


have_reference = P.have_reference


def build_ref_program(tmpdir):
    """tests/golden/cns_reads_ref_main.cpp against the reference's headers where they lie, linked with oracle/_ref/libref_cns_table.so"""
    exe = os.path.join(str(tmpdir), "cns_reads_ref")
    src = os.path.join(P.REF_ROOT, "src")
    subprocess.run(["g++", "-O2", "-w", "-pthread", "-fopenmp", "-I" + src, "-I" + os.path.join(src, "mecat2cns"), "-I" + os.path.join(src, "mecat2cns", "libboost"),
                    os.path.join(GOLDEN, "cns_reads_ref_main.cpp"), P.REF_LIB, "-Wl,-rpath," + os.path.dirname(P.REF_LIB), "-o", exe], check=True)
    return exe


def run_ref(exe, cases, tmpdir):
    """the reference's cns_results: per case a list of (id, range0, range1, seq bytes)"""
    fin, fout = os.path.join(str(tmpdir), "reads_cases.bin"), os.path.join(str(tmpdir), "reads_ref_out.bin")
    write_cases(fin, cases)
    subprocess.run([exe, fin, fout], check=True)
    data = open(fout, "rb").read()
    out, p = [], 0
    for _ in cases:
        n, = struct.unpack_from("<i", data, p)
        p += 4
        row = []
        for _ in range(n):
            rid, r0, r1, size = struct.unpack_from("<4i", data, p)
            row.append((rid, r0, r1, data[p + 16: p + 16 + size]))
            p += 16 + size
        out.append(row)
    assert p == len(data)
    return out


# ---- the exported split function (csrc/cns_reads.h through libcns_poa_host.so)

def host_split(size, beg, end):
    L = P.host_lib()
    L.cns_reads_host_blocks.restype = C.c_int64
    L.cns_reads_host_blocks.argtypes = [C.c_int64]
    L.cns_reads_host_block.restype = None
    L.cns_reads_host_block.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    o = (C.c_int64 * 4)()
    out = []
    for k in range(L.cns_reads_host_blocks(size)):
        L.cns_reads_host_block(size, k, beg, end, o)
        out.append(tuple(int(x) for x in o))
    return out


# ---- the fixture: inputs and recorded results only.  Explicit cases carry their letters and alignments and the reference's sequences;
# long cases carry their generator parameters, the reference's records and the SHA-256 of each record's letters.

def save_fixture(path, cases, results):
    ex = [c for c in cases if c["long"] is None]
    alns = [a for c in ex for a in c["alns"]]
    rec = [(r[0], r[1], r[2], len(r[3])) for row in results for r in row]
    is_long = np.array([c["long"] is not None for c in cases], dtype=np.uint8)
    np.savez_compressed(
        path,
        aln_q=np.frombuffer(b"".join(bytes(a[0]) for a in alns), dtype=np.uint8), aln_s=np.frombuffer(b"".join(bytes(a[1]) for a in alns), dtype=np.uint8),
        aln_len=np.array([len(a[0]) for a in alns], dtype=np.int32), aln_soff=np.array([a[2] for a in alns], dtype=np.int32),
        aln_send=np.array([a[3] for a in alns], dtype=np.int32), case_aln_begin=np.concatenate([[0], np.cumsum([len(c["alns"]) for c in ex])]).astype(np.int64),
        tmpl=np.frombuffer(b"".join(c["tmpl"] for c in ex), dtype=np.uint8), tmpl_begin=np.concatenate([[0], np.cumsum([len(c["tmpl"]) for c in ex])]).astype(np.int64),
        case_par=np.array([(c["tech"], c["min_cov"], c["min_size"], c["read_id"]) for c in cases], dtype=np.int32).reshape(-1, 4),
        case_long=is_long, long_par=np.array([c["long"] for c in cases if c["long"] is not None], dtype=np.int64).reshape(-1, 3),
        rec=np.array(rec, dtype=np.int32).reshape(-1, 4), case_rec_begin=np.concatenate([[0], np.cumsum([len(row) for row in results])]).astype(np.int64),
        seq=np.frombuffer(b"".join(r[3] for c, row in zip(cases, results) if c["long"] is None for r in row), dtype=np.uint8),
        sha=np.frombuffer(b"".join(hashlib.sha256(r[3]).digest() for c, row in zip(cases, results) if c["long"] is not None for r in row), dtype=np.uint8).reshape(-1, 32))


_fixture = None


def load_fixture():
    """-> (cases, results): per case the reference's records (id, range0, range1, letters — or, for a long case, (id, range0, range1, size,
    sha256 digest)); read once, shared, not to be changed"""
    global _fixture
    if _fixture is None:
        Z = np.load(FIXTURE)
        ab = np.concatenate([[0], np.cumsum(Z["aln_len"].astype(np.int64))])
        q, s, tm, seq = Z["aln_q"].tobytes(), Z["aln_s"].tobytes(), Z["tmpl"].tobytes(), Z["seq"].tobytes()
        cases, results = [], []
        e = li = sp = hp = 0
        for i, (tech, min_cov, min_size, rid) in enumerate(Z["case_par"].tolist()):
            r0, r1 = Z["case_rec_begin"][i: i + 2]
            if Z["case_long"][i]:
                c = long_case(*Z["long_par"][li].tolist())
                li += 1
                assert (c["tech"], c["min_cov"], c["min_size"], c["read_id"]) == (tech, min_cov, min_size, rid)
                row = []
                for a, b, d, size in Z["rec"][r0: r1].tolist():
                    row.append((a, b, d, size, Z["sha"][hp].tobytes()))
                    hp += 1
            else:
                a0, a1 = Z["case_aln_begin"][e: e + 2]
                alns = [(q[ab[a]: ab[a + 1]], s[ab[a]: ab[a + 1]], int(Z["aln_soff"][a]), int(Z["aln_send"][a])) for a in range(a0, a1)]
                c = case(tm[Z["tmpl_begin"][e]: Z["tmpl_begin"][e + 1]], alns, tech, min_cov, min_size, rid)
                e += 1
                row = []
                for a, b, d, size in Z["rec"][r0: r1].tolist():
                    row.append((a, b, d, seq[sp: sp + size]))
                    sp += size
            cases.append(c)
            results.append(row)
        _fixture = (cases, results)
    return _fixture


def same_as_recorded(got, row):
    """got: results_of(...) of one case; row: the fixture's records of it (letters or digests)"""
    if len(got) != len(row):
        return False
    for g, r in zip(got, row):
        if len(r) == 5:
            if g[:3] != r[:3] or len(g[3]) != r[3] or hashlib.sha256(g[3]).digest() != r[4]:
                return False
        elif g != tuple(r):
            return False
    return True
