#!/usr/bin/env python3
"""Golden vectors for mecat2ref's candidate stage (mecat_amd/csrc/ref_seed.hip, mecat_amd/host/ref_genome.cpp): the UNMODIFIED mecat2ref
with ref_cand_ref_main.cpp (next to this file) linked in place of its extend_candidate / rescue_clipped_align.  The reference's
mecat2ref and common sources are compiled where they lie into a temporary directory with oracle/Makefile's reference flags; nothing
compiled and no reference text is kept.  Build container only:
    python tests/golden/make_golden_ref_cand.py
Writes tests/golden/ref_cand.npz, data only: the reference FASTA, the reads (FASTA, one line per read), the chrindex.txt the tool wrote,
and per run (technology, -n) and round (1: 1 000-base segments, stride by length; 2: 2 000-base segments, stride 5) every read's
candidate list in call order — the recording extend_candidate returns false, so every read runs both rounds.  The script asserts, on
the reference alone, what the lists must show (the end of main) and stores the counts; "seconds" is the tool's own mapping time of
each run (one thread, extension stubbed out)."""
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cns_poa_cases as P  # noqa: E402
import helpers as H  # noqa: E402
import ref_cand_cases as RC  # noqa: E402

REF_ROOT = P.REF_ROOT
REFFLAGS = ["-D_GLIBCXX_PARALLEL", "-pthread", "-O3", "-w"]          # oracle/Makefile REFFLAGS / REFLINK
REFLINK = ["-pthread", "-lm", "-fopenmp"]
WEAK = ("extend_candidate", "rescue_clipped_align")

SEED = 20261
CHROMS = [(b"chrA first record", 26000), (b"chrB", 21000), (b"chrC\tthird", 13000)]
G = sum(n for _, n in CHROMS)
REPEAT = (3000, 2000, (12500, 31000, 49000))          # source, length, copies: four places in all
NPLANT, PLANT_COPIES = 5, 140
N_RUN = (8000, 60)
N_SINGLE = (17001, 40010)
R_AT = 52000
LOWER = (20000, 20700)


def build_ref_program(tmp):
    src = os.path.join(REF_ROOT, "src")
    files = [os.path.join(src, "mecat2ref", f) for f in ("mecat2ref.cpp", "mecat2ref_impl_large.cpp", "output.cpp", "mecat2ref_aux.cpp")]
    files += sorted(glob.glob(os.path.join(src, "common", "*.cpp")))
    objs = []
    for i, f in enumerate(files):
        o = os.path.join(tmp, "%d.o" % i)
        subprocess.run(["g++"] + REFFLAGS + ["-c", f, "-o", o], check=True)
        if os.path.basename(f) == "mecat2ref_aux.cpp":
            syms = [l.split()[-1] for l in subprocess.run(["nm", o], check=True, capture_output=True, text=True).stdout.splitlines()
                    if " T " in l and any(re.search(r"\d+%s" % w, l) for w in WEAK)]
            assert len(syms) == len(WEAK), syms
            subprocess.run(["objcopy"] + ["--weaken-symbol=" + s for s in syms] + [o], check=True)
        objs.append(o)
    rec = os.path.join(tmp, "rec.o")
    subprocess.run(["g++", "-O2", "-Wall", "-I" + os.path.join(src, "mecat2ref"), "-c", os.path.join(H.GOLDEN, "ref_cand_ref_main.cpp"), "-o", rec], check=True)
    exe = os.path.join(tmp, "mecat2ref_rec")
    subprocess.run(["g++"] + objs + [rec] + REFLINK + ["-o", exe], check=True)
    return exe


def kmer_count(g, km):
    w = np.lib.stride_tricks.sliding_window_view(g, 13)
    return int((w == km).all(axis=1).sum())


def make_reference():
    """-> (codes of the final genome, FASTA bytes, planted 13-mers)"""
    rng = np.random.default_rng(SEED)
    g = RC.genome(G, SEED)
    plants = [rng.integers(0, 4, 13).astype(np.uint8) for _ in range(NPLANT)]
    slots = rng.permutation(np.arange(100, G - 100, 40))[: NPLANT * PLANT_COPIES]          # sites 40 apart: no two overlap
    for i, s in enumerate(slots):
        g[s: s + 13] = plants[i % NPLANT]
    s0, ln, copies = REPEAT
    for c in copies:
        g[c: c + ln] = g[s0: s0 + ln]
    let = RC.letters(g).copy()
    let[N_RUN[0]: N_RUN[0] + N_RUN[1]] = ord("N")
    for p in N_SINGLE:
        let[p] = ord("N")
    let[R_AT] = ord("R")
    let[LOWER[0]: LOWER[1]] += 32
    seqs, p = [], 0
    for _, n in CHROMS:
        seqs.append(let[p: p + n])
        p += n
    return g, RC.fasta_bytes([n for n, _ in CHROMS], seqs, width=70), plants


def make_reads(g):
    """-> ([letters], {name: [read ids]})"""
    rng = np.random.default_rng(SEED + 1)
    reads, groups = [], {}

    def add(group, r, as_letters=False):          # r: codes 0..3, or letters
        groups.setdefault(group, []).append(len(reads))
        reads.append(r if as_letters else RC.letters(r).copy())

    def piece(a, b, err, idx):          # the genome's [a, b) as a read at error rate err, libsynth's choice of strand
        return RC.one_read(g[a:b], idx, b - a, err, SEED)
    # reads from anywhere, both strands, 0 - 15 % error
    for i in range(120):
        add("any", RC.one_read(g, i, int(rng.integers(300, 8001)), float(rng.choice([0.0, 0.03, 0.08, 0.12, 0.15])), SEED, ont=int(i % 2)))
    # error-free copies of 1 500 or more bases: segments overflow their 20 seeds
    for i in range(24):
        n = int(rng.integers(1500, 5000))
        a = int(rng.integers(0, G - n))
        add("exact", piece(a, a + n, 0.0, 1000 + i))
    # the reference's two ends
    add("head", piece(0, 2500, 0.0, 2000))
    add("head", piece(200, 3400, 0.10, 2001))
    add("head", piece(0, 900, 0.05, 2002))
    add("tail", piece(G - 3000, G, 0.0, 2003))
    add("tail", piece(G - 1800, G, 0.08, 2004))
    # chromosome boundaries, the N run, the repeat
    b1, b2 = CHROMS[0][1], CHROMS[0][1] + CHROMS[1][1]
    for i, (a, b, e) in enumerate([(b1 - 1500, b1 + 1800, 0.0), (b1 - 700, b1 + 2500, 0.10), (b2 - 2500, b2 + 900, 0.05), (b2 - 1000, b2 + 1000, 0.15)]):
        add("boundary", piece(a, b, e, 2100 + i))
    for i, (a, b, e) in enumerate([(N_RUN[0] - 1500, N_RUN[0] + 2000, 0.0), (N_RUN[0] - 600, N_RUN[0] + 3000, 0.10), (N_RUN[0] - 2500, N_RUN[0] + 400, 0.12)]):
        add("nrun", piece(a, b, e, 2200 + i))
    s0, ln, _ = REPEAT
    for i, e in enumerate([0.0, 0.05, 0.10, 0.12]):
        add("repeat", piece(s0 + 100, s0 + ln - 100, e, 2300 + i))
    add("repeat", piece(s0 - 800, s0 + ln + 700, 0.08, 2310))
    # lower-case and N letters of the reads' own (mecat2ref does not upper-case reads: such k-mers are skipped)
    for i in range(8):
        n = int(rng.integers(1500, 5000))
        a = int(rng.integers(0, G - n))
        r = RC.letters(piece(a, a + n, float(rng.choice([0.0, 0.05, 0.10])), 2400 + i)).copy()
        lo = int(rng.integers(0, len(r) - 400))
        if i % 2 == 0:
            r[lo: lo + 300] += 32
        for p in rng.integers(0, len(r), 1 + i):
            r[p] = ord("N")
        add("dirty", r, as_letters=True)
    # no source at all
    for i in range(10):
        add("random", rng.integers(0, 4, int(rng.integers(800, 4000))).astype(np.uint8))
    # the lengths at which the stride and the number of k-mers change
    for i, n in enumerate([12, 13, 17, 999, 1000]):
        add("len%d" % n, piece(30000 + 100 * i, 30000 + 100 * i + n, 0.0, 2500 + i))
    add("len15000", piece(18000, 33000, 0.0, 2510))
    add("len15000", piece(40000, 55000, 0.10, 2511)[:15000])
    for i in range(16):
        add("more", RC.one_read(g, 3000 + i, int(rng.integers(2000, 8001)), 0.15, SEED, ont=1))
    return reads, groups


def run(exe, tmp, ref_fa, reads_fa, tech, n):
    wd = os.path.join(tmp, "run_t%d_n%d" % (tech, n))
    os.makedirs(wd)
    rec = os.path.join(wd, "rec.bin")
    subprocess.run([exe, "-d", reads_fa, "-r", ref_fa, "-o", os.path.join(wd, "out.ref"), "-w", os.path.join(wd, "wrk"), "-t", "1", "-n", str(n), "-x", str(tech)],
                   check=True, cwd=wd, env=dict(os.environ, REF_CAND_OUT=rec), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    t = np.fromfile(rec, dtype=np.int64).reshape(-1, 12)
    secs = float(re.search(r"The Mapping Time: ([0-9.]+) sec", open(os.path.join(wd, "config.txt")).read()).group(1))
    return t, open(os.path.join(wd, "wrk", "chrindex.txt"), "rb").read(), secs


def split_rounds(t, nreads):
    """the record stream -> {round: [int64[count, 10] per read]}"""
    out = {1: [None] * nreads, 2: [None] * nreads}
    cur = []
    for row in t:
        if row[0] == 1:
            cur.append(row[1:12])
        else:
            rnd = {1000: 1, 2000: 2}[int(row[2])]
            rid = int(row[1])
            assert out[rnd][rid] is None and all(int(c[0]) == rid for c in cur)
            out[rnd][rid] = np.array(cur, dtype=np.int64).reshape(-1, 11)[:, 1:]
            cur = []
    assert not cur
    assert all(x is not None for r in (1, 2) for x in out[r]), "a read without both rounds"
    return out


def main():
    tmp = tempfile.mkdtemp(prefix="refcand_")
    exe = build_ref_program(tmp)
    g, ref_fa_bytes, plants = make_reference()
    reads, groups = make_reads(g)
    assert all(kmer_count(g, p) > 128 for p in plants), [kmer_count(g, p) for p in plants]
    assert sum(1 for r in groups["exact"] if len(reads[r]) >= 1500) >= 20
    ref_fa, reads_fa = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fa")
    open(ref_fa, "wb").write(ref_fa_bytes)
    reads_bytes = RC.fasta_bytes([b"r%d" % i for i in range(len(reads))], reads)
    open(reads_fa, "wb").write(reads_bytes)
    out = dict(ref_fasta=np.frombuffer(ref_fa_bytes, dtype=np.uint8), reads_fasta=np.frombuffer(reads_bytes, dtype=np.uint8),
               groups=np.array(json.dumps(groups)), plants=np.array(plants, dtype=np.uint8))
    lists, secs = {}, {}
    for tech, n in RC.RUNS:
        t, chrindex, s = run(exe, tmp, ref_fa, reads_fa, tech, n)
        if "chrindex" in out:
            assert out["chrindex"].tobytes() == chrindex
        out["chrindex"] = np.frombuffer(chrindex, dtype=np.uint8)
        secs["t%d_n%d" % (tech, n)] = s
        for rnd, per_read in split_rounds(t, len(reads)).items():
            key = "t%d_n%d_r%d" % (tech, n, rnd)
            lists[(tech, n, rnd)] = per_read
            out[key + "_counts"] = np.array([len(x) for x in per_read], dtype=np.int32)
            out[key + "_cands"] = np.concatenate(per_read).astype(np.int32)
            assert (out[key + "_cands"] == np.concatenate(per_read)).all()
    # ---- what the fixture must show (on the reference alone)
    shown = {}
    allc = np.concatenate([np.concatenate(v) for v in lists.values()])
    shown["chains"] = [int((allc[:, 9] == 0).sum()), int((allc[:, 9] == 1).sum())]
    assert min(shown["chains"]) >= 20
    shown["reads_with_2"] = sum(1 for x in lists[(0, 10, 1)] if len(x) >= 2)
    assert shown["reads_with_2"] >= 3
    shown["cut_at_3"] = sum(1 for tech in (0, 1) for rnd in (1, 2) for a, b in zip(lists[(tech, 10, rnd)], lists[(tech, 3, rnd)]) if len(a) > 3 and len(b) == 3)
    assert shown["cut_at_3"] >= 1
    for tech in (0, 1):
        for rnd in (1, 2):
            for a, b in zip(lists[(tech, 10, rnd)], lists[(tech, 3, rnd)]):
                assert (a[:3] == b).all()          # (-n 3 keeps the head of the -n 10 list unless candidates were dropped on the way)
    shown["round2_differs"] = sum(1 for a, b in zip(lists[(0, 10, 1)], lists[(0, 10, 2)]) if a.shape != b.shape or (a != b).any())
    assert shown["round2_differs"] >= 1
    shown["loc1_below_1000"] = int((allc[:, 0] < 1000).sum())
    assert shown["loc1_below_1000"] >= 1
    for v in lists.values():
        assert all(len(v[r]) == 0 for r in groups["random"])
        assert all(len(v[r]) == 0 for n in (12, 13, 17) for r in groups["len%d" % n])
    shown["nonempty"] = {"t%d_n%d_r%d" % k: sum(1 for x in v if len(x)) for k, v in lists.items()}
    shown["seconds"] = secs
    shown["reads"] = len(reads)
    shown["letters"] = int(sum(len(r) for r in reads))
    out["asserted"] = np.array(json.dumps(shown))
    print(shown, file=sys.stderr)
    np.savez_compressed(RC.FIXTURE + ".new.npz", **out)
    os.replace(RC.FIXTURE + ".new.npz", RC.FIXTURE)
    shutil.rmtree(tmp, ignore_errors=True)
    print("bytes", os.path.getsize(RC.FIXTURE), file=sys.stderr)


if __name__ == "__main__":
    main()
