#!/usr/bin/env python3
"""Golden vectors for mecat2ref's extension stage (mecat_amd/csrc/ref_extend.hip, mecat_amd/host/ref_results.cpp): the UNMODIFIED
extend_candidate (mecat2ref/mecat2ref_aux.cpp:123-183) with a DiffAligner, called by ref_ext_ref_main.cpp (next to this file) once per
candidate.  The reference's mecat2ref_aux.cpp, output.cpp and common sources are compiled where they lie into a temporary directory with
oracle/Makefile's reference flags; nothing compiled and no reference text is kept.  Build container only:
    python tests/golden/make_golden_ref_ext.py
Inputs are ref_cand.npz's: its reference, its reads, and the recorded PacBio -n 10 candidate lists of both rounds; to these come hand-made
candidates for the edges the lists may not hold (extend_candidate takes any candidate).  Writes tests/golden/ref_ext.npz, data only:
  cands [n, 5]     read, chain, loc1, loc2, score;   source [n]  1 / 2 = the round of the recorded list, 0 = hand-made
  res [n, 7]       ok, qb, qe, qs, sb, se, cols (sb / se of a result under 1 000 columns, which the tool does not form: the same expression,
                   ref_start - left_ref_size + target_start / target_end, from the aligner's coordinates)
  dirs [n, 2, 5]   per direction (left, right): columns, blocks, last block cut by the x 1.2 rule, kept blocks that ended at the best point,
                   most indel columns a tail anchor walked back over
  crc [n, 2]       CRC-32 of the query and the target string (ok results; 0 otherwise)
  stored, stored_offs, stored_words   the packed columns of a subset: every hand-made ok result and every eighth recorded one
For every ok result the strings rebuilt from columns + codes + coordinates (tests/ref_ext_ref.py: strings_of) must equal the tool's.  The
script asserts, on the reference alone, the cases the fixture must show (the end of main) and stores the counts; "go_seconds" is the
tool's own single-thread time in extend_candidate over all candidates."""
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zlib

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cns_poa_cases as P  # noqa: E402
import helpers as H  # noqa: E402
import make_golden_ref_cand as MC  # noqa: E402
import ref_cand_cases as RC  # noqa: E402
import ref_cand_ref as R  # noqa: E402
import ref_ext_cases as XC  # noqa: E402
import ref_ext_ref as X  # noqa: E402

REF_ROOT = P.REF_ROOT
REFFLAGS = MC.REFFLAGS
REFLINK = MC.REFLINK


def build_recorder(tmp):
    src = os.path.join(REF_ROOT, "src")
    files = [os.path.join(src, "mecat2ref", f) for f in ("output.cpp", "mecat2ref_aux.cpp")] + sorted(glob.glob(os.path.join(src, "common", "*.cpp")))
    objs = []
    for i, f in enumerate(files):
        o = os.path.join(tmp, "%d.o" % i)
        subprocess.run(["g++"] + REFFLAGS + ["-c", f, "-o", o], check=True)
        objs.append(o)
    rec = os.path.join(tmp, "rec.o")
    subprocess.run(["g++", "-O2", "-Wall", "-I" + os.path.join(src, "mecat2ref"), "-c", os.path.join(H.GOLDEN, "ref_ext_ref_main.cpp"), "-o", rec], check=True)
    exe = os.path.join(tmp, "ref_ext_rec")
    subprocess.run(["g++", rec] + objs + REFLINK + ["-o", exe], check=True)
    return exe


def hand_made(base, reads, G):
    """candidates off the recorded ones: (read, chain, loc1, loc2, score) -> list; every one stays inside the reference and the read"""
    groups = json.loads(str(base["groups"]))
    first = {}          # read -> its first recorded candidate of round 1
    for rid, lst in enumerate(RC.recorded(base, 0, 10, 1)):
        if len(lst):
            first[rid] = lst[0]
    out = []

    def shifted(rid, d, dref=0):          # the read's first candidate moved d bases along its diagonal (and dref more on the reference)
        c = first[rid]
        l1, l2 = int(c[0]) + d + dref, int(c[1]) + d
        if 1 <= l1 <= G and 0 <= l2 < len(reads[rid]):
            out.append((rid, int(c[9]), l1, l2, int(c[6])))
    for g in ("head", "tail", "exact", "boundary", "nrun", "dirty", "repeat", "len999", "len1000"):
        for rid in groups.get(g, []):
            if rid not in first:
                continue
            c = first[rid]
            L = len(reads[rid])
            shifted(rid, -int(c[1]))                          # read_start = 0: an empty left direction
            shifted(rid, -min(int(c[1]), int(c[0]) - 1))      # the window's left end on the reference's first base, or read_start = 0
            shifted(rid, L - 1 - int(c[1]))                   # one query base to the right
            shifted(rid, min(L - 1 - int(c[1]), G - int(c[0])))
            shifted(rid, 1 - int(c[1]))                       # a left direction of one base
            for side in (599, 600, 601, 718):                 # block-size edges on the left
                shifted(rid, side - int(c[1]))
    # the repeat's other copies: the read fits for the repeat's length only, the directions end at a best point
    s0, ln, copies = MC.REPEAT
    for rid in groups["repeat"]:
        if rid in first:
            for a in (s0,) + tuple(copies):
                for b in (s0,) + tuple(copies):
                    if a != b:
                        shifted(rid, 0, b - a)
    return sorted(set(out))


def main():
    base = RC.fixture()
    reads = base["read_list"]
    let, _ = R.read_reference(base["ref_fasta"].tobytes())
    let = R.upper(let)
    codes = X.ENCODE[let]
    G = len(let)
    cands, source = [], []
    for rnd in (1, 2):
        for rid, lst in enumerate(RC.recorded(base, 0, 10, rnd)):
            for c in lst:
                cands.append((rid, int(c[9]), int(c[0]), int(c[1]), int(c[6])))
                source.append(rnd)
    n_rec = (source.count(1), source.count(2))
    assert n_rec == (575, 1060), n_rec
    hm = hand_made(base, reads, G)
    cands += hm
    source += [0] * len(hm)
    cands = np.array(cands, dtype=np.int64)
    source = np.array(source, dtype=np.int32)
    n = len(cands)

    tmp = tempfile.mkdtemp(prefix="refext_")
    exe = build_recorder(tmp)
    inp, outp, strp = (os.path.join(tmp, f) for f in ("in.bin", "out.bin", "str.bin"))
    with open(inp, "wb") as f:
        np.array([G, len(reads), n], dtype=np.int64).tofile(f)
        f.write(let.tobytes())
        for r in reads:
            np.array([len(r)], dtype=np.int64).tofile(f)
            f.write(np.asarray(r, dtype=np.uint8).tobytes())
        cands.tofile(f)
    subprocess.run([exe, inp, outp, strp], check=True)
    rec = np.fromfile(outp, dtype=np.int64).reshape(n, 20)
    strings = []
    with open(strp, "rb") as f:
        for i in range(n):
            c = int(np.fromfile(f, dtype=np.int64, count=1)[0])
            strings.append((f.read(c), f.read(c)))
    shutil.rmtree(tmp, ignore_errors=True)

    res = np.zeros((n, 7), dtype=np.int64)
    dirs = np.zeros((n, 2, 5), dtype=np.int64)
    crc = np.zeros((n, 2), dtype=np.uint32)
    stored, stored_offs, stored_words = [], [0], []
    n_ok_rec = 0
    shown = dict(candidates=[int(x) for x in n_rec] + [len(hm)])
    lower_n_rev = 0
    for i in range(n):
        rid, chain, loc1, loc2, _ = (int(x) for x in cands[i])
        ok, qb, qe, qs, ts, te, cols, lcols, rcols, sb, se = (int(x) for x in rec[i, :11])
        ref_start, read_start, left, right = X.window(G, len(reads[rid]), loc1, loc2)
        if ok:
            assert (sb, se) == (ref_start - left + ts, ref_start - left + te)
        sb, se = ref_start - left + ts, ref_start - left + te
        assert ok == int(cols >= 1000) and qs == len(reads[rid]) and cols == lcols + rcols == len(strings[i][0])
        res[i] = (ok, qb, qe, qs, sb, se, cols)
        dirs[i, 0] = (lcols,) + tuple(rec[i, 11:15])
        dirs[i, 1] = (rcols,) + tuple(rec[i, 15:19])
        if not ok:
            continue
        qm, sm = strings[i]
        crc[i] = (zlib.crc32(qm), zlib.crc32(sm))
        words = X.columns_of(qm, sm)
        strand = X.ENCODE[X.strand_letters(reads[rid], chain)]
        q2, s2, qe2, se2 = X.strings_of(words, cols, strand, codes, qb, sb)
        assert (q2, s2, qe2, se2) == (qm, sm, qe, se), ("rebuilt strings differ", i)
        if source[i] == 0 or n_ok_rec % 8 == 0:
            stored.append(i)
            stored_words.append(words)
            stored_offs.append(stored_offs[-1] + len(words))
        n_ok_rec += source[i] != 0
        if chain:          # a lower-case stretch and an N of the read inside the aligned region, on the reverse strand
            region = X.strand_letters(reads[rid], 1)[qb:qe]
            low = (region >= ord("a")) & (region <= ord("z"))
            if low.sum() >= 100 and (region == ord("N")).any():
                lower_n_rev += 1

    # ---- what the fixture must show (on the reference alone)
    ok = res[:, 0] == 1
    shown["chains"] = [int((cands[:, 1] == 0).sum()), int((cands[:, 1] == 1).sum())]
    shown["ok_by_chain"] = [int((ok & (cands[:, 1] == 0)).sum()), int((ok & (cands[:, 1] == 1)).sum())]
    assert min(shown["ok_by_chain"]) >= 20
    shown["ok"], shown["under_1000"] = int(ok.sum()), int((~ok).sum())
    assert shown["ok"] >= 100 and shown["under_1000"] >= 20
    shown["under_1000_with_columns"] = int((~ok & (res[:, 6] > 0)).sum())
    assert shown["under_1000_with_columns"] >= 5
    d = dirs.reshape(-1, 5)
    kept = d[:, 0] > 0
    shown["dirs_one_block"] = int((kept & (d[:, 1] == 1)).sum())
    shown["dirs_several_blocks"] = int((kept & (d[:, 1] >= 3)).sum())
    shown["dirs_last_block_sized"] = int((kept & (d[:, 2] == 1)).sum())
    shown["dirs_best_point"] = int((kept & (d[:, 3] >= 1)).sum())
    shown["dirs_tail_over_16_rows"] = int((kept & (d[:, 4] > 16)).sum())
    for k in ("dirs_one_block", "dirs_several_blocks", "dirs_last_block_sized", "dirs_best_point", "dirs_tail_over_16_rows"):
        assert shown[k] >= 1, (k, shown)
    win = np.array([X.window(G, len(reads[int(c[0])]), int(c[2]), int(c[3])) for c in cands], dtype=np.int64)
    ref_start, read_start, left, right = win.T
    shown["empty_left"] = int((read_start == 0).sum())
    shown["empty_left_ok"] = int(((read_start == 0) & ok).sum())
    assert shown["empty_left_ok"] >= 1
    shown["left_of_one_base"] = int((np.minimum(read_start, left) == 1).sum())
    rlen = res[:, 3]
    shown["clipped_first_base"] = int(((left == ref_start) & ((np.minimum(read_start, ref_start) * 1.2).astype(np.int64) > ref_start) & (res[:, 6] > 0)).sum())
    shown["clipped_last_base"] = int(((right == G - ref_start) & ((np.minimum(rlen - read_start, G - ref_start) * 1.2).astype(np.int64) > G - ref_start) & (res[:, 6] > 0)).sum())
    assert shown["clipped_first_base"] >= 1 and shown["clipped_last_base"] >= 1
    shown["reaches_first_base"] = int((ok & (res[:, 4] == 0)).sum())
    shown["reaches_last_base"] = int((ok & (res[:, 5] == G)).sum())
    assert shown["reaches_first_base"] >= 1 and shown["reaches_last_base"] >= 1
    b1, b2 = MC.CHROMS[0][1], MC.CHROMS[0][1] + MC.CHROMS[1][1]
    shown["across_chromosomes"] = int((ok & (((res[:, 4] < b1 - 50) & (res[:, 5] > b1 + 50)) | ((res[:, 4] < b2 - 50) & (res[:, 5] > b2 + 50)))).sum())
    shown["across_n_run"] = int((ok & (res[:, 4] < MC.N_RUN[0] - 50) & (res[:, 5] > MC.N_RUN[0] + MC.N_RUN[1] + 50)).sum())
    assert shown["across_chromosomes"] >= 1 and shown["across_n_run"] >= 1
    shown["lower_case_and_n_on_reverse"] = lower_n_rev
    assert lower_n_rev >= 1
    shown["go_seconds"] = float(rec[:, 19].sum()) * 1e-9
    shown["query_bases_aligned"] = int((res[:, 2] - res[:, 1]).sum())
    shown["stored"] = len(stored)
    print(shown, file=sys.stderr)
    out = dict(cands=cands.astype(np.int32), source=source.astype(np.int8), res=res.astype(np.int32), dirs=dirs.astype(np.int16), crc=crc,
               stored=np.array(stored, dtype=np.int32), stored_offs=np.array(stored_offs, dtype=np.int64), stored_words=np.concatenate(stored_words),
               asserted=np.array(json.dumps(shown)))
    for k in ("cands", "res", "dirs"):
        assert (out[k] == {"cands": cands, "res": res, "dirs": dirs}[k]).all()
    np.savez_compressed(XC.FIXTURE + ".new.npz", **out)
    os.replace(XC.FIXTURE + ".new.npz", XC.FIXTURE)
    print("bytes", os.path.getsize(XC.FIXTURE), file=sys.stderr)


if __name__ == "__main__":
    main()
