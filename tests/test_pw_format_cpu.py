"""format_can_read / format_m4_read (mecat_amd/host/pw_format.h: what the mecat2pw driver makes of one read's candidates and extension
results) against the oracle's restatement of the reference (orc_m4_fill -> orc_m4_postfilter -> orc_m4_line, pinned to the reference by
test_oracle_vs_ref.py; helpers.can_lines_from_cands for `.can`), read by read, byte for byte and in order: both sides sort with
libstdc++'s std::sort and the same comparator on the same input order.  tests/pw_format_check.cpp is a stand-alone program built with
AddressSanitizer and UndefinedBehaviorSanitizer; nothing is loaded into this process but the oracle.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H

NQ, NREF, Q_START, REF_START = 300, 12, 1000, 57          # (non-zero start_read_id on both volumes)
EDGES = (-101, -100, -99, -1, 0, 1, 99, 100, 101)          # around the 100-base containment margin


def _cases():
    """-> (q_sizes, ref_sizes, per read: list of (readno, chain, loc1, loc2, score, ok, qs, qe, ts, te, matches, columns))"""
    rng = np.random.RandomState(20261019)
    q_sizes = rng.randint(4000, 20000, NQ)
    ref_sizes = rng.randint(4000, 20000, NREF)
    reads = []
    for r in range(NQ):
        kind = r % 10
        nbase = 0 if kind == 0 else rng.randint(8, 12) if kind == 5 else rng.randint(1, 5)
        recs = []
        for _ in range(nbase):
            s = rng.randint(0, 3 if kind == 5 else NREF)          # few subjects: several records for one subject
            chain = rng.randint(0, 2)
            tlen = rng.randint(500, 2500)
            ts = rng.randint(200, ref_sizes[s] - tlen - 200)
            qs = rng.randint(200, q_sizes[r] - tlen - 200)
            variants = [(0, 0, 0, 0, chain)]
            for _ in range(3 if kind == 5 else rng.randint(0, 4)):
                d = [EDGES[rng.randint(0, len(EDGES))] for _ in range(4)]
                if rng.randint(0, 3) == 0:
                    d[1], d[3] = d[0], d[2]          # the interval shifted as a whole: equal (qid, overlap size) keys
                variants.append((d[0], d[1], d[2], d[3], chain if rng.randint(0, 4) else 1 - chain))      # same and opposite directions
            for d0, d1, d2, d3, ch in variants:
                loc1 = 0 if rng.randint(0, 6) == 0 else rng.randint(1, ref_sizes[s])
                loc2 = 0 if rng.randint(0, 6) == 0 else rng.randint(1, q_sizes[r])
                columns = 0 if rng.randint(0, 20) == 0 else tlen + rng.randint(0, 300)
                matches = 0 if columns == 0 else rng.randint(columns // 2, columns + 1)
                ok = 0 if kind == 1 else int(rng.randint(0, 8) != 0)
                recs.append((REF_START + s, ch, loc1, loc2, rng.randint(1, 60), ok, qs + d2, qs + tlen + d3, ts + d0, ts + tlen + d1, matches, columns))
        reads.append(recs)
    return q_sizes, ref_sizes, reads


def _half_kmer(loc2, loc1):
    return (loc2 + 6, loc1 + 6) if loc2 and loc1 else (loc2, loc1)          # pw_impl.cpp:681-685


def _expected(q_sizes, ref_sizes, reads, mode):
    q_offs = np.stack([np.zeros(NQ, dtype=np.int64), q_sizes], axis=1)
    ref_offs = np.stack([np.zeros(NREF, dtype=np.int64), ref_sizes], axis=1)
    want = []
    if mode == "can":
        for r, recs in enumerate(reads):
            a = np.zeros(len(recs), dtype=H.CAND_DTYPE)
            for k, t in enumerate(recs):
                a[k]["readno"], a[k]["chain"], a[k]["loc1"], a[k]["loc2"], a[k]["score"] = t[:5]
            got = H.can_lines_from_cands([a], q_offs[r:r + 1], ref_offs, 0, REF_START)
            want.append([ln.replace("%d\t" % 0, "%d\t" % (r + Q_START), 1) for ln in got])          # (the helper numbers its reads from its own 0)
        return want
    O = H.orc()
    buf = C.create_string_buffer(512)
    for r, recs in enumerate(reads):
        m4v = (H.OrcM4 * max(1, len(recs)))()
        k = 0
        for readno, chain, loc1, loc2, score, ok, qs, qe, ts, te, matches, columns in recs:
            if not ok:
                continue
            qstart, sstart = _half_kmer(loc2, loc1)
            ar = H.OrcAlnResult(ok, qs, qe, ts, te, matches, columns)
            O.orc_m4_fill(C.byref(ar), r + Q_START, readno, b"R" if chain else b"F", int(q_sizes[r]), int(ref_sizes[readno - REF_START]), qstart, sstart,
                          score, C.byref(m4v[k]))
            k += 1
        out = (H.OrcM4 * max(1, k))()
        kept = O.orc_m4_postfilter(m4v, k, out)
        lines = []
        for j in range(kept):
            n = O.orc_m4_line(C.byref(out[j]), 1 if mode == "m4g1" else 0, buf)
            lines.append(buf.raw[:n].decode().rstrip("\n"))
        want.append(lines)
    return want


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("pw_format")
    exe = str(d / "pw_format_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(H.ROOT, "include"), "-I" + os.path.join(H.ROOT, "mecat_amd", "host"),
                    os.path.join(H.ROOT, "tests", "pw_format_check.cpp"), "-o", exe], check=True)
    q_sizes, ref_sizes, reads = _cases()
    case = str(d / "cases.txt")
    with open(case, "w") as f:
        f.write("%d %d %d %d\n%s\n%s\n" % (NQ, Q_START, NREF, REF_START, " ".join(map(str, q_sizes)), " ".join(map(str, ref_sizes))))
        for recs in reads:
            f.write("%d\n" % len(recs) + "".join(" ".join(map(str, t)) + "\n" for t in recs))
    return exe, case, (q_sizes, ref_sizes, reads)


def test_cases_cover_the_edges(checker):
    _, _, (q_sizes, ref_sizes, reads) = checker
    oks = [[t for t in recs if t[5]] for recs in reads]
    assert any(not recs for recs in reads) and any(recs and not o for recs, o in zip(reads, oks))          # no candidate; all ok == 0
    assert {t[1] for recs in reads for t in recs} == {0, 1}
    assert any(t[2] == 0 and t[3] for recs in reads for t in recs) and any(t[3] == 0 and t[2] for recs in reads for t in recs)
    assert any(t[11] == 0 and t[5] for recs in reads for t in recs)
    big = [o for o in oks if len(o) > 16]
    assert big and any(len({(t[0], min(t[7] - t[6], t[9] - t[8])) for t in o}) < len(o) for o in big)          # equal (qid, overlap size) keys


@pytest.mark.parametrize("mode", ["can", "m4g0", "m4g1"])
def test_lines_equal_the_oracles_read_by_read(checker, mode):
    exe, case, (q_sizes, ref_sizes, reads) = checker
    r = subprocess.run([exe, case, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-2000:]
    got = [blk.rstrip("\n").split("\n")[1:] for blk in ("\n" + out).split("\n== ")[1:]]
    want = _expected(q_sizes, ref_sizes, reads, mode)
    assert len(got) == len(want) == NQ
    for r_, (g, w) in enumerate(zip(got, want)):
        assert g == w, "read %d" % r_
    assert sum(len(w) for w in want) > 300
    if mode != "can":          # the post-filter removed records, and kept several of one subject
        assert sum(len(w) for w in want) < sum(1 for recs in reads for t in recs if t[5])
