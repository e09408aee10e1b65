#!/usr/bin/env python3
"""Golden vectors for mecat2ref's extension stage in nanopore mode (mecat_amd/csrc/ref_xextend.hip, mecat_amd/host/ref_results.cpp): the
UNMODIFIED extend_candidate (mecat2ref/mecat2ref_aux.cpp:123-183) with an XdropAligner, called by ref_xext_ref_main.cpp (next to this
file) once per candidate, and the whole unmodified tool at `-x 1` on the rescue chain's reads.  The reference's sources are compiled where
they lie into a temporary directory with oracle/Makefile's reference flags; nothing compiled and no reference text is kept.  Build
container only:
    python tests/golden/make_golden_ref_xext.py
Inputs (tests/ref_xext_cases.py): set 0 = ref_cand.npz's reference and reads with its recorded `-x 1 -n 10` lists of both rounds and
make_golden_ref_ext.hand_made's candidates; set 1 = second_set(): the low-complexity reference with reads across it, and the crafted
every-fourth-base pairs.  Writes tests/golden/ref_xext.npz, data only:
  cands [n, 5]     read, chain, loc1, loc2, score;  set [n] 0 / 1;  source [n]  1 / 2 = the round of the recorded list, 0 = hand-made,
                   3 = low-complexity, 4 = crafted
  res [n, 8]       ok, qb, qe, qs, sb, se, cols, matches (sb / se of a result that is not ok, which the tool does not form: the same
                   expression, ref_start - left_ref_size + target_start / target_end, from the aligner's coordinates)
  dirs [n, 2, 5]   per direction (left, right) as align_ex leaves it: columns, blocks, last block cut by the x 1.2 rule, ended by X-drop
                   before the block's end, ended by a failed trim
  crc [n, 2]       CRC-32 of the query and the target string (ok results; 0 otherwise)
  stored, stored_offs, stored_words   the packed columns of a subset: every crafted, low-complexity and hand-made ok result and every
                   eighth recorded one
  tool_x_reads, tool_x_read_lens   the chain's extra reads (tests/ref_xext_cases.py: extra_chain_reads), behind ref_rescue.npz's tool_reads
  tool_x_n<N>_b<B> the record streams of the whole tool at -x 1 (tests/golden/ref_rescue_ref_main.cpp's tool mode, as ref_rescue.npz's)
For every ok result the strings rebuilt from columns + codes + coordinates (tests/ref_ext_ref.py: strings_of) must equal the tool's.  The
script asserts, on the reference alone, the cases the fixture must show (the end of main) and stores the counts; "go_seconds" is the
tool's own single-thread time in extend_candidate over all candidates."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zlib

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import helpers as H  # noqa: E402
import make_golden_ref_cand as MC  # noqa: E402
import make_golden_ref_ext as MXE  # noqa: E402
import make_golden_ref_rescue as MR  # noqa: E402
import ref_cand_cases as RC  # noqa: E402
import ref_cand_ref as R  # noqa: E402
import ref_ext_ref as X  # noqa: E402
import ref_rescue_cases as SC  # noqa: E402
import ref_xext_cases as XX  # noqa: E402


def build_recorder(tmp):
    import glob
    src = os.path.join(MXE.REF_ROOT, "src")
    files = [os.path.join(src, "mecat2ref", f) for f in ("output.cpp", "mecat2ref_aux.cpp")] + sorted(glob.glob(os.path.join(src, "common", "*.cpp")))
    objs = []
    for i, f in enumerate(files):
        o = os.path.join(tmp, "%d.o" % i)
        subprocess.run(["g++"] + MXE.REFFLAGS + ["-c", f, "-o", o], check=True)
        objs.append(o)
    rec = os.path.join(tmp, "rec.o")
    subprocess.run(["g++", "-O2", "-Wall", "-I" + os.path.join(src, "mecat2ref"), "-c", os.path.join(H.GOLDEN, "ref_xext_ref_main.cpp"), "-o", rec], check=True)
    exe = os.path.join(tmp, "ref_xext_rec")
    subprocess.run(["g++", rec] + objs + MXE.REFLINK + ["-o", exe], check=True)
    return exe


def record(exe, tmp, tag, let, reads, cands):
    """one set through the recorder -> (rec int64[n, 21], [(qmap, smap)])"""
    n = len(cands)
    inp, outp, strp = (os.path.join(tmp, tag + f) for f in ("in.bin", "out.bin", "str.bin"))
    with open(inp, "wb") as f:
        np.array([len(let), len(reads), n], dtype=np.int64).tofile(f)
        f.write(let.tobytes())
        for r in reads:
            np.array([len(r)], dtype=np.int64).tofile(f)
            f.write(np.asarray(r, dtype=np.uint8).tobytes())
        np.asarray(cands, dtype=np.int64).tofile(f)
    subprocess.run([exe, inp, outp, strp], check=True)
    rec = np.fromfile(outp, dtype=np.int64).reshape(n, 21)
    strings = []
    with open(strp, "rb") as f:
        for i in range(n):
            c = int(np.fromfile(f, dtype=np.int64, count=1)[0])
            strings.append((f.read(c), f.read(c)))
    return rec, strings


def record_tool(tmp, base, codes, out, shown):
    """the chain reads of tests/ref_rescue_cases.py through the whole tool at -x 1 -> out["tool_x_n%d_b%d"] and what the runs show"""
    exe = MR.build_tool(tmp)
    extra = XX.extra_chain_reads(codes)
    reads = SC.chain_reads(codes) + extra
    out["tool_x_reads"] = np.concatenate(extra)
    out["tool_x_read_lens"] = np.array([len(r) for r in extra], dtype=np.int32)
    ref_fa, reads_fa = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fa")
    open(ref_fa, "wb").write(base["ref_fasta"].tobytes())
    open(reads_fa, "wb").write(RC.fasta_bytes([b"r%d" % i for i in range(len(reads))], reads))
    seen = dict(calls=0, early_return=0, left_attach=0, right_attach=0, extended_not_attached=0, rescue_candidates=0, extend_failed=0, round2_calls=0)
    for n, b in XX.TOOL_RUNS:
        wd = os.path.join(tmp, "xrun_n%d_b%d" % (n, b))
        os.makedirs(wd)
        rec = os.path.join(wd, "rec.bin")
        subprocess.run([exe, "-d", reads_fa, "-r", ref_fa, "-o", os.path.join(wd, "out.ref"), "-w", os.path.join(wd, "wrk"), "-t", "1", "-n", str(n), "-b", str(b),
                        "-x", "1"], check=True, cwd=wd, env=dict(os.environ, REF_RESCUE_OUT=rec), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        t = np.fromfile(rec, dtype="<i8")
        out["tool_x_n%d_b%d" % (n, b)] = t
        calls = SC.parse_tool_stream(t)
        assert {c["read"] for c in calls} == set(range(len(reads)))
        for c in calls:
            added = c["nres1"] - c["nres0"]
            att = [a for a in c["after"] if a[8] != -1]
            seen["calls"] += 1
            seen["round2_calls"] += c["block_size"] == 2000
            seen["rescue_candidates"] += len(c["extends"])
            seen["extend_failed"] += sum(1 for e in c["extends"] if not e[4])
            seen["early_return"] += bool(len(c["after"]) and c["after"][0][1] - c["after"][0][0] >= c["read_len"] * 0.9 and not c["finds"])
            seen["left_attach"] += sum(1 for a in c["after"] if a[6] != -1)
            seen["right_attach"] += sum(1 for a in c["after"] if a[7] != -1)
            # extended (ok or not) and not attached: every extension of the call that did not end as an attached entry
            seen["extended_not_attached"] += max(0, len(c["extends"]) - len(att)) if not (added and len(c["after"]) < c["naln0"]) else 0
    shown["tool"] = seen
    print(seen, file=sys.stderr)
    for k in ("early_return", "left_attach", "right_attach", "extended_not_attached"):
        assert seen[k] >= 1, (k, seen)


def main():
    base = RC.fixture()
    reads0 = base["read_list"]
    let0, _ = R.read_reference(base["ref_fasta"].tobytes())
    let0 = R.upper(let0)
    cands, source = [], []
    for rnd in (1, 2):
        for rid, lst in enumerate(RC.recorded(base, 1, 10, rnd)):
            for c in lst:
                cands.append((rid, int(c[9]), int(c[0]), int(c[1]), int(c[6])))
                source.append(rnd)
    n_rec = (source.count(1), source.count(2))
    hm = MXE.hand_made(base, reads0, len(let0))
    cands += hm
    source += [0] * len(hm)
    text1, reads1, cands1, source1 = XX.second_set()
    let1, _ = R.read_reference(text1)
    let1 = R.upper(let1)
    sets = [(let0, reads0), (let1, reads1)]
    n0 = len(cands)
    cands = np.concatenate([np.array(cands, dtype=np.int64), cands1])
    source = np.concatenate([np.array(source, dtype=np.int64), source1.astype(np.int64)])
    which = np.concatenate([np.zeros(n0, dtype=np.int64), np.ones(len(cands1), dtype=np.int64)])
    n = len(cands)

    tmp = tempfile.mkdtemp(prefix="refxext_")
    exe = build_recorder(tmp)
    rec0, str0 = record(exe, tmp, "a", let0, reads0, cands[:n0])
    rec1, str1 = record(exe, tmp, "b", let1, reads1, cands[n0:])
    rec = np.concatenate([rec0, rec1])
    strings = str0 + str1

    res = np.zeros((n, 8), dtype=np.int64)
    dirs = np.zeros((n, 2, 5), dtype=np.int64)
    crc = np.zeros((n, 2), dtype=np.uint32)
    stored, stored_offs, stored_words = [], [0], []
    n_ok_rec = 0
    shown = dict(candidates=[int(x) for x in n_rec] + [len(hm), int((source == XX.SRC_LOWC).sum()), int((source == XX.SRC_CRAFT).sum())])
    lower_n_rev = 0
    codes = [X.ENCODE[let0], X.ENCODE[let1]]
    for i in range(n):
        let, reads = sets[which[i]]
        G = len(let)
        rid, chain, loc1, loc2, _ = (int(x) for x in cands[i])
        ok, qb, qe, qs, ts, te, cols, lraw, rraw, sb, se, matches = (int(x) for x in rec[i, :12])
        ref_start, read_start, left, right = X.window(G, len(reads[rid]), loc1, loc2)
        if ok:
            assert (sb, se) == (ref_start - left + ts, ref_start - left + te)
        sb, se = ref_start - left + ts, ref_start - left + te
        assert ok == int(qe - qb >= 1000) and qs == len(reads[rid]) and cols == max(lraw - 1, 0) + rraw == len(strings[i][0])
        res[i] = (ok, qb, qe, qs, sb, se, cols, matches)
        dirs[i, 0] = (lraw,) + tuple(rec[i, 12:16])
        dirs[i, 1] = (rraw,) + tuple(rec[i, 16:20])
        if not ok:
            continue
        qm, sm = strings[i]
        crc[i] = (zlib.crc32(qm), zlib.crc32(sm))
        words = XX.columns_of(qm, sm)
        strand = X.ENCODE[X.strand_letters(reads[rid], chain)]
        q2, s2, qe2, se2 = X.strings_of(words, cols, strand, codes[which[i]], qb, sb)
        assert (q2, s2, qe2, se2) == (qm, sm, qe, se), ("rebuilt strings differ", i)
        if source[i] not in (1, 2) or n_ok_rec % 8 == 0:
            stored.append(i)
            stored_words.append(words)
            stored_offs.append(stored_offs[-1] + len(words))
        n_ok_rec += source[i] in (1, 2)
        if chain and which[i] == 0:          # a lower-case stretch and an N of the read inside the aligned region, on the reverse strand
            region = X.strand_letters(reads[rid], 1)[qb:qe]
            low = (region >= ord("a")) & (region <= ord("z"))
            if low.sum() >= 100 and (region == ord("N")).any():
                lower_n_rev += 1

    # ---- what the fixture must show (on the reference alone)
    ok = res[:, 0] == 1
    nat = which == 0          # the natural candidates: the recorded lists and the hand-made ones
    span = res[:, 2] - res[:, 1]
    shown["natural"], shown["recorded"] = int(nat.sum()), int(sum(n_rec))
    shown["ok"] = int((ok & nat).sum())
    shown["ok_by_chain"] = [int((ok & nat & (cands[:, 1] == 0)).sum()), int((ok & nat & (cands[:, 1] == 1)).sum())]
    assert min(shown["ok_by_chain"]) >= 100, shown
    shown["not_ok_with_columns"] = int((~ok & nat & (res[:, 6] > 0)).sum())
    assert shown["not_ok_with_columns"] >= 20, shown
    shown["columns_ge_1000_span_lt_1000"] = int((nat & (res[:, 6] >= 1000) & (span < 1000)).sum())
    assert shown["columns_ge_1000_span_lt_1000"] >= 10, shown
    shown["span_990_1010"] = int((nat & (span >= 990) & (span <= 1010)).sum())
    assert shown["span_990_1010"] >= 5, shown
    d = dirs[nat].reshape(-1, 5)
    shown["dirs_xdrop_end"] = int((d[:, 3] == 1).sum())
    assert shown["dirs_xdrop_end"] >= 100, shown
    shown["dirs_one_block"] = int(((d[:, 0] > 0) & (d[:, 1] == 1)).sum())
    shown["dirs_three_or_more_blocks"] = int(((d[:, 0] > 0) & (d[:, 1] >= 3)).sum())
    shown["dirs_last_block_sized"] = int(((d[:, 0] > 0) & (d[:, 2] == 1)).sum())
    assert min(shown["dirs_one_block"], shown["dirs_three_or_more_blocks"], shown["dirs_last_block_sized"]) >= 1, shown
    shown["left_of_one_column"] = int((nat & (dirs[:, 0, 0] == 1)).sum())
    assert shown["left_of_one_column"] >= 5, shown
    shown["empty_left"] = int((nat & (dirs[:, 0, 0] == 0)).sum())
    shown["empty_left_ok"] = int((nat & ok & (dirs[:, 0, 0] == 0)).sum())
    assert shown["empty_left_ok"] >= 1, shown
    shown["failed_trim_natural"] = int((d[:, 4] == 1).sum())
    shown["failed_trim"] = int((dirs[:, :, 4] == 1).sum())
    shown["failed_trim_in_second_block"] = int(((dirs[:, :, 4] == 1) & (dirs[:, :, 1] == 2)).sum())
    assert shown["failed_trim"] >= 1 and shown["failed_trim_in_second_block"] >= 1, shown
    shown["low_complexity_ok"] = int((ok & (source == XX.SRC_LOWC)).sum())
    assert shown["low_complexity_ok"] >= 1, shown
    shown["crafted_ok"] = int((ok & (source == XX.SRC_CRAFT)).sum())
    shown["mismatch_columns"] = int((res[ok, 6] - res[ok, 7]).sum())          # columns of unequal letters in the ok results, gap columns among them
    # stage 2's geometric cases (set 0)
    G = len(let0)
    win = np.array([X.window(G, len(reads0[int(c[0])]), int(c[2]), int(c[3])) for c in cands[:n0]], dtype=np.int64)
    ref_start, read_start, left, right = win.T
    r0, ok0 = res[:n0], ok[:n0]
    shown["clipped_first_base"] = int(((left == ref_start) & ((np.minimum(read_start, ref_start) * 1.2).astype(np.int64) > ref_start) & (r0[:, 6] > 0)).sum())
    shown["clipped_last_base"] = int(((right == G - ref_start) & ((np.minimum(r0[:, 3] - read_start, G - ref_start) * 1.2).astype(np.int64) > G - ref_start) & (r0[:, 6] > 0)).sum())
    assert shown["clipped_first_base"] >= 1 and shown["clipped_last_base"] >= 1, shown
    b1, b2 = MC.CHROMS[0][1], MC.CHROMS[0][1] + MC.CHROMS[1][1]
    shown["across_chromosomes"] = int((ok0 & (((r0[:, 4] < b1 - 50) & (r0[:, 5] > b1 + 50)) | ((r0[:, 4] < b2 - 50) & (r0[:, 5] > b2 + 50)))).sum())
    shown["across_n_run"] = int((ok0 & (r0[:, 4] < MC.N_RUN[0] - 50) & (r0[:, 5] > MC.N_RUN[0] + MC.N_RUN[1] + 50)).sum())
    assert shown["across_chromosomes"] >= 1 and shown["across_n_run"] >= 1, shown
    shown["lower_case_and_n_on_reverse"] = lower_n_rev
    assert lower_n_rev >= 1
    shown["go_seconds"] = float(rec[:n0, 20].sum()) * 1e-9
    shown["stored"] = len(stored)
    print(shown, file=sys.stderr)
    out = dict(cands=cands.astype(np.int32), set=which.astype(np.int8), source=source.astype(np.int8), res=res.astype(np.int32), dirs=dirs.astype(np.int16), crc=crc,
               stored=np.array(stored, dtype=np.int32), stored_offs=np.array(stored_offs, dtype=np.int64), stored_words=np.concatenate(stored_words))
    for k in ("cands", "res", "dirs"):
        assert (out[k] == {"cands": cands, "res": res, "dirs": dirs}[k]).all()
    record_tool(tmp, base, codes[0], out, shown)
    shutil.rmtree(tmp, ignore_errors=True)
    out["asserted"] = np.array(json.dumps(shown))
    np.savez_compressed(XX.FIXTURE + ".new.npz", **out)
    os.replace(XX.FIXTURE + ".new.npz", XX.FIXTURE)
    size = os.path.getsize(XX.FIXTURE)
    print("bytes", size, file=sys.stderr)
    assert size <= os.path.getsize(os.path.join(H.GOLDEN, "ref_cand.npz")), "thin the stored columns (never the CRCs)"


if __name__ == "__main__":
    main()
