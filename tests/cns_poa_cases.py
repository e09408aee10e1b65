"""Inputs and plumbing for the POA tests (test_cns_poa_ref_cpu.py, test_gpu_cns_poa.py, golden/make_golden_cns_poa.py): cases of one
template each — alignments (qaln, saln, soff, send) as in cns_pieces_cases, windows (sb, se, cov), and `fresh`: every window gets newly
added alignments (fresh cursors) instead of the cursors the windows in front of it left.  Hand-written cases, seeded random ones from
cns_pieces_cases' generator with a cov column, templates whose alignments agree with each other, windows with 100 pieces, and the
threshold case.  Also here: the packed case file both C++ programs read, the fixture's arrays, the host routine (libcns_poa_host.so)
through ctypes, and the census of what the cases make the graph do, read off the host routine's own counters."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import cns_pieces_cases as K
import cns_pieces_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "cns_poa.npz")
REF_ROOT = "/root/reference"
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libref_cns_table.so")
MAGIC = 0x504F4131
GAP = Q.GAP
FIXTURE_SEED, FRESH_SEED = 20264, 20265


def case(alns, windows, fresh=False):
    return dict(alns=list(alns), windows=[tuple(int(x) for x in w) for w in windows], fresh=bool(fresh))


def hand_cases():
    a = K.aln
    out = [
        case([], [(3, 9, 0), (9, 11, 4), (20, 320, 0)]),                                   # no pieces: N..N at minWeight 0, "" above
        case([a("ACGTA", 10)], [(8, 12, 0), (12, 14, 1), (14, 16, 3)]),
        case([a("ACGTA", 10), a("ACGTA", 10), a("ACGTA", 10)], [(10, 11, 3), (11, 14, 8)]),   # blen 2; min weight 3 of weight 4
        case([a("AC--GT-A", 0, "ACTTG-TA"), a("AC--GT-A", 0, "ACTTGTTA"), a("AC-GTA", 0, "ACTGTA")], [(0, 2, 2), (2, 3, 2), (3, 5, 2)]),
        case([a("A---C", 5, "ATTTC"), a("A---C", 5, "ATTTC"), a("A--C", 5, "ATTC"), a("AC", 5)], [(5, 6, 4)]),      # insertion runs, merged
        case([a("-AC-G", 10, "TACTG"), a("-AC-G", 10, "TACTG")], [(10, 12, 2), (12, 13, 2)]),                      # saln[0] a gap
        case([a("ACG", 0, "AGG"), a("ACG", 0, "A-G"), a("ACG", 0, "ACG")], [(0, 2, 2)]),                            # a column with two letters
        case([a("ACGT", 0, "A--T"), a("ACGT", 0, "A--T"), a("ACGT", 0)], [(0, 3, 3)]),                              # deletions outvote
        case([a("A-C", 0, "AGC"), a("A-C", 0, "ATC"), a("A-C", 0, "AGC"), a("A-C", 0, "ATC")], [(0, 1, 4)]),        # a tie of two insertions
        case([a("AC", 0, "--"), a("AC", 0, "A-")], [(0, 1, 1)]),
    ]
    return out


def threshold_cases():
    """two cases on fresh cursors, a window per cov 0 .. 255.  First: 100 alignments of 2 .. 101 matching columns at position 0 and the
    window (0, 101): the best path has the weights 101, 101, 100, 99, .. 2 (the longest alignment's last edge goes to '$' past the last
    backbone vertex), so the consensus is as long as the vertices with weight >= (int)(cov * 0.4): every threshold 2 .. 102 gives another
    length.  Second: no alignment and the window (0, 5): six vertices of weight 1, "NNNNNN" up to a threshold of 1 and "" from 2 on.
    (0 and 1 cannot be told apart by any graph: no vertex on a path has weight 0.)"""
    return [case([K.aln("A" * n, 0) for n in range(2, 102)], [(0, 101, cov) for cov in range(256)], fresh=True),
            case([], [(0, 5, cov) for cov in range(256)], fresh=True)]


def with_cov(rng, windows, n_alns):
    top = max(1, n_alns)
    return [(sb, se, int(rng.choice([0, 1, 2, 3, top, int(rng.integers(0, 2 * top + 3)), int(rng.integers(0, 256))]))) for sb, se in windows]


def agreeing_case(rng, L, n_alns, pe, whole=False):
    """alignments that copy one template, with query gaps, insertions (runs too) and their ends anywhere; windows between anchors"""
    tmpl = rng.choice(list(b"ACGT"), L)
    windows = K.random_windows(rng, L, rng.random() < 0.7)
    alns = []
    for _ in range(n_alns):
        soff = int(rng.integers(0, max(1, L // 3))) if rng.random() < 0.5 and not whole else 0
        end = L if rng.random() < 0.5 or whole else int(rng.integers(soff + 1, L + 1))
        q, s = bytearray(), bytearray()
        for p in range(soff, end):
            if p > soff and rng.random() < pe:
                for _ in range(int(rng.choice([1, 1, 1, 2, 3, 4]))):
                    q.append(int(rng.choice(list(b"ACGT")))); s.append(GAP)
            s.append(int(tmpl[p]))
            q.append(GAP if rng.random() < pe else int(tmpl[p]))
        alns.append((bytes(q), bytes(s), soff, end))
    return case(alns, with_cov(rng, windows, n_alns))


def random_cases(seed, count):
    """a third each: cns_pieces_cases' generator (alignments that need not agree), agreeing alignments, and small dense ones; every
    50th case has 100 alignments over short windows, every other one of them with all alignments over the whole template"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        if i % 50 == 49:
            out.append(agreeing_case(rng, int(rng.integers(6, 16)), 100, 0.15, whole=i % 100 == 49))
        elif i % 3 == 0:
            alns, windows = K.random_case(rng, int(rng.integers(4, 70)), 6, 40)
            out.append(case(alns, with_cov(rng, windows, len(alns))))
        elif i % 3 == 1:
            out.append(agreeing_case(rng, int(rng.integers(4, 60)), int(rng.integers(1, 13)), float(rng.choice([0.05, 0.15, 0.3]))))
        else:
            out.append(agreeing_case(rng, int(rng.integers(3, 12)), int(rng.integers(2, 30)), float(rng.choice([0.15, 0.3, 0.5]))))
    return out


def pieces_of(c):
    """(pieces [Q.PIECE_DTYPE], piece_begin) as meap_cns_one_indel's loop gets them (cns_pieces_ref.retrieve_literal, the cursor)"""
    wins = [(sb, se) for sb, se, _ in c["windows"]]
    if not c["fresh"]:
        return Q.retrieve_literal(c["alns"], wins)
    parts = [Q.retrieve_literal(c["alns"], [w])[0] for w in wins]
    pb = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, Q.PIECE_DTYPE)), pb


def write_cases(path, cases, tails=None):
    """the packed case file: int32 MAGIC, cases, has_tail; per case: fresh, alignments, per alignment soff, send, len and the bytes of
    qaln and saln; windows, per window sb, se, cov; with tails [(pieces, piece_begin, strings)]: piece_begin [windows + 1] as int32, the
    piece records, per window the length and bytes of its recorded string"""
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", MAGIC, len(cases), int(tails is not None)))
        for i, c in enumerate(cases):
            f.write(struct.pack("<2i", int(c["fresh"]), len(c["alns"])))
            for q, s, soff, send in c["alns"]:
                f.write(struct.pack("<3i", soff, send, len(q)) + bytes(q) + bytes(s))
            f.write(struct.pack("<i", len(c["windows"])))
            f.write(np.array(c["windows"], dtype="<i4").reshape(-1, 3).tobytes())
            if tails is not None:
                pieces, pb, strings = tails[i]
                f.write(np.asarray(pb, dtype="<i4").tobytes())
                f.write(np.ascontiguousarray(pieces).view("<i4").tobytes())
                for s in strings:
                    f.write(struct.pack("<i", len(s)) + bytes(s))


def have_reference():
    return os.path.isdir(os.path.join(REF_ROOT, "src")) and os.path.exists(REF_LIB)


def build_ref_program(tmpdir):
    """tests/golden/cns_poa_ref_main.cpp against the reference's headers where they lie, linked with oracle/_ref/libref_cns_table.so"""
    exe = os.path.join(str(tmpdir), "cns_poa_ref")
    src = os.path.join(REF_ROOT, "src")
    subprocess.run(["g++", "-O2", "-w", "-pthread", "-fopenmp", "-I" + src, "-I" + os.path.join(src, "mecat2cns"), "-I" + os.path.join(src, "mecat2cns", "libboost"),
                    os.path.join(GOLDEN, "cns_poa_ref_main.cpp"), REF_LIB, "-Wl,-rpath," + os.path.dirname(REF_LIB), "-o", exe], check=True)
    return exe


def run_ref(exe, cases, tmpdir):
    """the reference's strings: a list per case"""
    fin, fout = os.path.join(str(tmpdir), "cases.bin"), os.path.join(str(tmpdir), "ref_out.bin")
    write_cases(fin, cases)
    subprocess.run([exe, fin, fout], check=True)
    data = open(fout, "rb").read()
    out, p = [], 0
    for c in cases:
        row = []
        for _ in c["windows"]:
            n, = struct.unpack_from("<i", data, p)
            row.append(data[p + 4: p + 4 + n])
            p += 4 + n
        out.append(row)
    assert p == len(data)
    return out


# ---- the host routine

INFO_NAMES = ("rc", "bound_nodes", "bound_edges", "nodes", "edges", "queue", "frames", "members", "in_merges", "in_recursive", "out_merges", "exists", "ties", "stops_early")
_host = None


def host_lib_path():
    return os.path.join(ROOT, "mecat_amd", "lib", "libcns_poa_host.so")


def host_lib():
    global _host
    if _host is None:
        L = C.CDLL(host_lib_path())
        L.cns_poa_host_case.restype = C.c_int
        L.cns_poa_host_case.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.cns_poa_host_words.restype = C.c_int64
        L.cns_poa_host_words.argtypes = [C.c_int64, C.c_int64]
        L.cns_poa_host_min_weight.argtypes = [C.c_int]
        _host = L
    return _host


def pack_alns(alns):
    """mhip_debug_push_gaps' layout: qaln + NUL + saln + NUL per alignment -> (buf, off, len, soff, send)"""
    off, parts, p = [], [], 0
    for q, s, _, _ in alns:
        off.append(p)
        parts += [bytes(q), b"\0", bytes(s), b"\0"]
        p += 2 * (len(q) + 1)
    buf = np.frombuffer(b"".join(parts) or b"\0", dtype=np.uint8).copy()
    return (buf, np.array(off, dtype=np.int64), np.array([len(a[0]) for a in alns], dtype=np.int32), np.array([a[2] for a in alns], dtype=np.int32),
            np.array([a[3] for a in alns], dtype=np.int32))


def host_run_packed(buf, off, ln, windows, pieces, pb):
    """libcns_poa_host.so on one template -> (cns bytes uint8, cns_begin int64 [windows + 1], info [windows, len(INFO_NAMES)])"""
    L = host_lib()
    win = np.ascontiguousarray(np.asarray(windows, dtype=np.int32).reshape(-1, 3))
    pieces = np.ascontiguousarray(pieces)
    pb = np.ascontiguousarray(pb, dtype=np.int64)
    cap = int(sum(int(se) - int(sb) + 3 for sb, se, _ in win) + (pieces["ncols"].sum() if len(pieces) else 0)) + 16
    out = np.zeros(cap, np.uint8)
    ob = np.zeros(len(win) + 1, np.int64)
    info = np.zeros((len(win), len(INFO_NAMES)), np.int32)
    rc = L.cns_poa_host_case(buf.ctypes.data, off.ctypes.data, ln.ctypes.data, len(ln), win.ctypes.data, len(win), pieces.ctypes.data, pb.ctypes.data, out.ctypes.data, cap,
                             ob.ctypes.data, info.ctypes.data)
    assert rc == 0, "cns_poa_host_case returned %d" % rc
    return out[: ob[-1]], ob, info


def host_run(c, pieces=None, pb=None):
    """-> (the windows' strings as a list of bytes, info)"""
    if pieces is None:
        pieces, pb = pieces_of(c)
    buf, off, ln, _, _ = pack_alns(c["alns"])
    out, ob, info = host_run_packed(buf, off, ln, c["windows"], pieces, pb)
    return [out[ob[w]: ob[w + 1]].tobytes() for w in range(len(c["windows"]))], info


# ---- the census

SITUATIONS = ("no_pieces", "blen2", "starts_inside", "one_column_piece", "insertion_run3", "leading_gap_column", "in_merge_recursive", "out_merge", "exists", "tie",
              "stops_early", "cns_le2", "pieces100", "uncovered_position")


def census(c, pieces, pb, strings, info, count):
    """adds one case's windows to count (a dict over SITUATIONS): one per window that shows the situation"""
    col = {n: i for i, n in enumerate(INFO_NAMES)}
    for w, (sb, se, cov) in enumerate(c["windows"]):
        pc = pieces[pb[w]: pb[w + 1]]
        count["no_pieces"] += len(pc) == 0
        count["blen2"] += se - sb + 1 == 2
        count["pieces100"] += len(pc) == 100
        count["cns_le2"] += len(strings[w]) <= 2
        covered = np.zeros(se - sb + 2, bool)
        inside = one = run3 = lead = False
        for p in pc:
            q, s, _, _ = c["alns"][int(p["aln"])]
            a, n = int(p["col"]), int(p["ncols"])
            qq, ss = q[a: a + n], s[a: a + n]
            inside |= int(p["sb_out"]) > sb
            one |= n == 1
            lead |= ss[0] == GAP
            run, pos = 0, int(p["sb_out"]) - sb
            for x, y in zip(qq, ss):
                run = run + 1 if (y == GAP and x != GAP) else (run if (x == GAP and y == GAP) else 0)
                run3 |= run >= 3
                if y != GAP:
                    if pos < len(covered):
                        covered[pos] = True
                    pos += 1
        count["starts_inside"] += inside
        count["one_column_piece"] += one
        count["insertion_run3"] += run3
        count["leading_gap_column"] += lead
        count["uncovered_position"] += len(pc) > 0 and not covered[: se - sb + 1].all()
        count["in_merge_recursive"] += info[w, col["in_recursive"]] > 0
        count["out_merge"] += info[w, col["out_merges"]] > 0
        count["exists"] += info[w, col["exists"]] > 0
        count["tie"] += info[w, col["ties"]] > 0
        count["stops_early"] += info[w, col["stops_early"]] > 0


# ---- the fixture

def save_fixture(path, cases, strings):
    alns = [a for c in cases for a in c["alns"]]
    np.savez_compressed(
        path,
        aln_q=np.frombuffer(b"".join(bytes(a[0]) for a in alns), dtype=np.uint8), aln_s=np.frombuffer(b"".join(bytes(a[1]) for a in alns), dtype=np.uint8),
        aln_len=np.array([len(a[0]) for a in alns], dtype=np.int32), aln_soff=np.array([a[2] for a in alns], dtype=np.int32),
        aln_send=np.array([a[3] for a in alns], dtype=np.int32), case_aln_begin=np.concatenate([[0], np.cumsum([len(c["alns"]) for c in cases])]).astype(np.int64),
        windows=np.array([w for c in cases for w in c["windows"]], dtype=np.int32).reshape(-1, 3),
        case_win_begin=np.concatenate([[0], np.cumsum([len(c["windows"]) for c in cases])]).astype(np.int64), case_fresh=np.array([c["fresh"] for c in cases], dtype=np.uint8),
        cns=np.frombuffer(b"".join(s for row in strings for s in row), dtype=np.uint8),
        cns_begin=np.concatenate([[0], np.cumsum([len(s) for row in strings for s in row])]).astype(np.int64))


_fixture = None


def load_fixture():
    """-> (cases, strings): the recorded reference strings, a list per case (read once, shared, not to be changed)"""
    global _fixture
    if _fixture is None:
        Z = np.load(FIXTURE)
        ab = np.concatenate([[0], np.cumsum(Z["aln_len"].astype(np.int64))])
        q, s = Z["aln_q"].tobytes(), Z["aln_s"].tobytes()
        cases, strings = [], []
        cns, cb = Z["cns"].tobytes(), Z["cns_begin"]
        for i in range(len(Z["case_fresh"])):
            a0, a1 = Z["case_aln_begin"][i: i + 2]
            w0, w1 = Z["case_win_begin"][i: i + 2]
            alns = [(q[ab[a]: ab[a + 1]], s[ab[a]: ab[a + 1]], int(Z["aln_soff"][a]), int(Z["aln_send"][a])) for a in range(a0, a1)]
            cases.append(case(alns, Z["windows"][w0: w1], Z["case_fresh"][i]))
            strings.append([cns[cb[w]: cb[w + 1]] for w in range(w0, w1)])
        _fixture = (cases, strings)
    return _fixture
