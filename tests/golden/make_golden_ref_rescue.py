#!/usr/bin/env python3
"""Golden vectors for mecat2ref's rescue stage (mecat_amd/csrc/ref_rescue.hip): the UNMODIFIED rescue_clipped_align
(mecat2ref/mecat2ref_aux.cpp:308-452) and output_results (:454-473), called by ref_rescue_ref_main.cpp (next to this file) on the
hand-made cases of tests/ref_rescue_cases.py.  The reference's mecat2ref_aux.cpp, output.cpp and common sources are compiled where they
lie into a temporary directory with oracle/Makefile's reference flags; output_temp_result is weakened in output.o so that the recorder's
own takes its place and notes which result is printed.  Nothing compiled and no reference text is kept.  Build container only:
    python tests/golden/make_golden_ref_rescue.py
Writes tests/golden/ref_rescue.npz, data only: the cases' inputs (reads as letters, entries, segment records) and per case what the two
calls left: the AlignInfo array, the number of results, the fields of the results the call added with the CRC-32 of their two strings,
and the ids in the order output_results printed them.  The reference is ref_cand.npz's.  The script asserts, on the reference alone,
which branches the cases reached (the end of main) and stores the counts."""
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
import make_golden_ref_cand as MC  # noqa: E402
import ref_cand_cases as RC  # noqa: E402
import ref_ext_cases as XC  # noqa: E402
import ref_rescue_cases as SC  # noqa: E402

REF_ROOT = P.REF_ROOT


def build_recorder(tmp):
    src = os.path.join(REF_ROOT, "src")
    files = [os.path.join(src, "mecat2ref", f) for f in ("output.cpp", "mecat2ref_aux.cpp")] + sorted(glob.glob(os.path.join(src, "common", "*.cpp")))
    objs = []
    for i, f in enumerate(files):
        o = os.path.join(tmp, "%d.o" % i)
        subprocess.run(["g++"] + MC.REFFLAGS + ["-c", f, "-o", o], check=True)
        if os.path.basename(f) == "output.cpp":
            syms = [l.split()[-1] for l in subprocess.run(["nm", o], check=True, capture_output=True, text=True).stdout.splitlines()
                    if " T " in l and re.search(r"\d+output_temp_result", l)]
            assert len(syms) == 1, syms
            subprocess.run(["objcopy", "--weaken-symbol=" + syms[0], o], check=True)
        objs.append(o)
    rec = os.path.join(tmp, "rec.o")
    subprocess.run(["g++", "-O2", "-Wall", "-I" + os.path.join(src, "mecat2ref"), "-c", os.path.join(H.GOLDEN, "ref_rescue_ref_main.cpp"), "-o", rec], check=True)
    exe = os.path.join(tmp, "ref_rescue_rec")
    subprocess.run(["g++", rec] + objs + MC.REFLINK + ["-o", exe], check=True)
    return exe


INNER = ("extend_candidate", "fill_clipped_candidate", "find_left_clipped_candidate", "find_right_clipped_candidate")


def build_tool(tmp):
    """the whole unmodified mecat2ref with the recorder's two functions around rescue_clipped_align and output_results"""
    src = os.path.join(REF_ROOT, "src")
    files = [os.path.join(src, "mecat2ref", f) for f in ("mecat2ref.cpp", "mecat2ref_impl_large.cpp", "output.cpp", "mecat2ref_aux.cpp")]
    files += sorted(glob.glob(os.path.join(src, "common", "*.cpp")))
    objs = []
    for i, f in enumerate(files):
        o = os.path.join(tmp, "t%d.o" % i)
        subprocess.run(["g++"] + MC.REFFLAGS + ["-c", f, "-o", o], check=True)
        if os.path.basename(f) == "mecat2ref_aux.cpp":
            # as position-independent code: calls between the file's global functions go through their symbols, so the recorder's
            # functions can stand between them (checked below on the relocations)
            subprocess.run(["g++"] + MC.REFFLAGS + ["-fPIC", "-c", f, "-o", o], check=True)
            names = subprocess.run(["nm", o], check=True, capture_output=True, text=True).stdout.splitlines()
            mangled = {}
            for w in ("rescue_clipped_align", "output_results") + INNER:
                syms = [l.split()[-1] for l in names if " T " in l and re.search(r"^_Z\d+%s" % w, l.split()[-1])]
                assert len(syms) == 1, (w, syms)
                mangled[w] = syms[0]
            relocs = subprocess.run(["readelf", "-rW", o], check=True, capture_output=True, text=True).stdout
            for w in INNER:
                assert mangled[w] in relocs, "no call of %s through its symbol" % w
            # a copy per function the originals are called from: that function under the name orig_*, every definition weak, so that
            # the copy's own calls of the other three still reach the recorder's functions
            for w in INNER:
                o2 = os.path.join(tmp, "t%d_%s.o" % (i, w))
                subprocess.run(["objcopy", "--redefine-sym", "%s=orig_%s" % (mangled[w], w), "--weaken", o, o2], check=True)
                objs.append(o2)
            subprocess.run(["objcopy"] + [a for w in ("rescue_clipped_align", "output_results") for a in ("--redefine-sym", "%s=orig_%s" % (mangled[w], w))]
                           + ["--weaken-symbol=" + mangled[w] for w in INNER] + [o], check=True)
        objs.append(o)
    rec = os.path.join(tmp, "trec.o")
    subprocess.run(["g++", "-O2", "-Wall", "-Wno-unused-function", "-DREF_RESCUE_TOOL", "-I" + os.path.join(src, "mecat2ref"), "-c",
                    os.path.join(H.GOLDEN, "ref_rescue_ref_main.cpp"), "-o", rec], check=True)
    exe = os.path.join(tmp, "mecat2ref_rec")
    subprocess.run(["g++"] + objs + [rec] + MC.REFLINK + ["-o", exe], check=True)
    return exe


def run_tool(exe, tmp, ref_fa, reads_fa, n, b):
    wd = os.path.join(tmp, "run_n%d_b%d" % (n, b))
    os.makedirs(wd)
    rec = os.path.join(wd, "rec.bin")
    subprocess.run([exe, "-d", reads_fa, "-r", ref_fa, "-o", os.path.join(wd, "out.ref"), "-w", os.path.join(wd, "wrk"), "-t", "1", "-n", str(n), "-b", str(b), "-x", "0"],
                   check=True, cwd=wd, env=dict(os.environ, REF_RESCUE_OUT=rec), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return np.fromfile(rec, dtype="<i8")


def record_tool(tmp, base, codes, out, shown):
    """the chain reads of tests/ref_rescue_cases.py through the whole tool at -n 1, 2, 10 and -b 1, 10 -> out["tool_n%d_b%d"], the record
    streams as the recorder writes them, and the counts of what they show"""
    exe = build_tool(tmp)
    reads = SC.chain_reads(codes)
    ref_fa, reads_fa = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fa")
    open(ref_fa, "wb").write(base["ref_fasta"].tobytes())
    open(reads_fa, "wb").write(RC.fasta_bytes([b"r%d" % i for i in range(len(reads))], reads))
    out["tool_reads"] = np.concatenate(reads)
    out["tool_read_lens"] = np.array([len(r) for r in reads], dtype=np.int32)
    seen = dict(calls=0, early_return=0, left_attach=0, right_attach=0, ok_unattached=0, rescue_on_R=0, rescue_round2=0, containment_removals=0,
                more_than_three=0, num_output_cuts=0, full_cut=0, round2_calls=0, no_location=0, best_score2_le_4=0, gate_read_side=0, gate_ref_side=0,
                score2_over_20=0, extend_failed=0, rescue_candidates=0)
    for n, b in SC.TOOL_RUNS:
        t = run_tool(exe, tmp, ref_fa, reads_fa, n, b)
        out["tool_n%d_b%d" % (n, b)] = t
        calls = SC.parse_tool_stream(t)
        assert {c["read"] for c in calls} == set(range(len(reads)))
        for c in calls:
            added = c["nres1"] - c["nres0"]
            att = [a for a in c["after"] if a[8] != -1]
            seen["calls"] += 1
            for side, gr, gf, filled, sc2, fret, ret in c["finds"]:
                seen["gate_read_side"] += gr
                seen["gate_ref_side"] += int(gf and not gr)
                seen["best_score2_le_4"] += int(not gr and not gf and not filled)
                seen["no_location"] += int(filled and not fret)
                seen["score2_over_20"] += int(filled and sc2 > 20)
                assert ret == (filled and fret) and (not filled or sc2 > 4)
            seen["rescue_candidates"] += len(c["extends"])
            seen["extend_failed"] += sum(1 for e in c["extends"] if not e[4])
            assert sum(1 for e in c["extends"] if e[4]) == added and len(c["extends"]) == sum(1 for x in c["finds"] if x[6])
            seen["round2_calls"] += c["block_size"] == 2000
            seen["early_return"] += bool(len(c["after"]) and c["after"][0][1] - c["after"][0][0] >= c["read_len"] * 0.9 and added == 0)
            seen["left_attach"] += sum(1 for a in c["after"] if a[6] != -1)
            seen["right_attach"] += sum(1 for a in c["after"] if a[7] != -1)
            seen["ok_unattached"] += added - len(att) if added and not (len(c["after"]) < c["naln0"] + len(att)) else 0
            seen["rescue_on_R"] += sum(1 for r in c["results"][c["nres0"]:] if r[1] == 1)
            seen["rescue_round2"] += added if c["block_size"] == 2000 else 0
            seen["containment_removals"] += max(0, c["naln0"] - (len(c["after"]) - len(att))) if added == len(att) else 0
            seen["more_than_three"] += len(c["after"]) - len(att) > 3
            seen["num_output_cuts"] += sum(1 for a in c["after"] if a[8] == -1) > b
            seen["full_cut"] += bool(added and len(c["after"]) < c["naln0"] and all(a[8] == -1 for a in c["after"])
                                     and c["after"][-1][1] - c["after"][-1][0] >= c["read_len"] * 0.9 and any(a[5] >= c["nres0"] for a in c["after"]))
    shown["tool"] = seen
    print(seen, file=sys.stderr)
    for k in ("early_return", "left_attach", "right_attach", "ok_unattached", "rescue_on_R", "containment_removals", "more_than_three", "num_output_cuts",
              "no_location", "best_score2_le_4", "gate_read_side", "gate_ref_side", "score2_over_20", "rescue_round2"):
        assert seen[k] >= 1, (k, seen)
    # what these reads do not reach in the whole tool (no attached result covers 0.9 of its read): shown by the hand-made cases above only
    shown["hand_made_only"] = [k for k in ("rescue_round2", "full_cut") if seen[k] == 0]
    assert len(shown["hand_made_only"]) <= 2


def main():
    tmp = tempfile.mkdtemp(prefix="refrescue_")
    exe = build_recorder(tmp)
    base = RC.fixture()
    _, U = XC.ref_codes(base["ref_fasta"].tobytes())
    cases = SC.make_cases(U)
    w = lambda v: np.asarray(v, dtype="<i8").tobytes()
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(w([len(U), len(cases)]) + U.tobytes() + b"".join(SC.case_input_words(c) for c in cases))
    subprocess.run([exe, fin, fout], check=True)
    t = np.fromfile(fout, dtype="<i8")
    at = 0

    def take(n):
        nonlocal at
        v = t[at: at + n]
        assert len(v) == n
        at += n
        return v
    reads, read_of, meta = [], {}, []
    for c in cases:
        naln, nres = (int(x) for x in take(2))
        after = take(naln * len(SC.AFTER_FIELDS)).reshape(naln, len(SC.AFTER_FIELDS))
        new = take((nres - len(c["entries"])) * len(SC.NEW_FIELDS)).reshape(-1, len(SC.NEW_FIELDS))
        printed = take(int(take(1)[0]))
        key = c["read"].tobytes()
        if key not in read_of:
            read_of[key] = len(reads)
            reads.append(c["read"])
        meta.append(dict(name=c["name"], read=read_of[key], block_size=c["block_size"], bc=c["bc"], num_output=c["num_output"], entries=c["entries"],
                         fwd={str(s): list(v) for s, v in c["fwd"].items()}, rev={str(s): list(v) for s, v in c["rev"].items()},
                         after=after.tolist(), nresults=nres, new=new.tolist(), printed=printed.tolist()))
    assert at == len(t)
    # ---- what the fixture must show (on the reference alone)
    by = {m["name"]: m for m in meta}
    F = {n: i for i, n in enumerate(SC.AFTER_FIELDS)}
    added = lambda m: m["nresults"] - len(m["entries"])
    attached = lambda m, side: sum(1 for a in m["after"] if a[F["prev_id" if side == 0 else "next_id"]] != -1)
    shown = dict(cases=len(meta))
    shown["early_return"] = int(added(by["full_edge_19800"]) == 0 and added(by["full_edge_19799"]) == 1)
    shown["left_attach"] = sum(attached(m, 0) for m in meta)
    shown["right_attach"] = sum(attached(m, 1) for m in meta)
    shown["ok_unattached"] = sum(added(m) - sum(1 for a in m["after"] if a[F["parent_id"]] != -1) for m in meta if m["name"] != "full_cut")
    shown["no_location"] = int(added(by["right_no_location"]) == 0)
    shown["score2_gate"] = int(added(by["right_score2_4"]) == 0 and added(by["right_score2_5"]) == 0 and added(by["right_score2_6"]) == 1)
    shown["gate_read_side"] = int(added(by["right_gate_read_3700"]) == 0 and added(by["right_gate_read_3699"]) == 1 and added(by["left_gate_read_2000"]) == 0
                                  and added(by["left_gate_read_2001"]) == 1)
    shown["gate_ref_side"] = int(added(by["right_gate_ref_2000"]) == 0 and added(by["right_gate_ref_2001"]) == 1 and added(by["left_gate_ref_2000"]) == 0
                                 and added(by["left_gate_ref_2001"]) == 1)
    shown["score2_over_20"] = int(added(by["right_score2_25"]) == 1)
    shown["rescue_on_R"] = sum(1 for m in meta for r in m["new"] if r[1] == 1)
    shown["rescue_round2"] = int(added(by["right_attach_round2"]) == 1)
    shown["containment_removals"] = sum(len(m["entries"]) - len(m["after"]) for m in meta if not m["fwd"] and not m["rev"])
    shown["fourth_not_rescued"] = int(added(by["fourth_not_tried"]) == 3)
    shown["num_output_cuts"] = sum(1 for m in meta if sum(1 for a in m["after"] if a[F["parent_id"]] == -1) > m["num_output"])
    shown["full_cut"] = int(len(by["full_cut"]["after"]) == 1 and by["full_cut"]["printed"] == [1])
    shown["tie_winner_by_vscore"] = [by["right_attach"]["new"][0][0], by["right_larger_wins"]["new"][0][0], by["left_attach_R"]["new"][0][0], by["left_tie_R"]["new"][0][0]]
    print(shown, file=sys.stderr)
    if os.environ.get("REF_RESCUE_SHOW"):
        for m in meta:
            print(m["name"], m["entries"], "->", m["after"], m["nresults"], m["new"], m["printed"], file=sys.stderr)
    for k in ("early_return", "left_attach", "right_attach", "ok_unattached", "no_location", "score2_gate", "gate_read_side", "gate_ref_side", "score2_over_20",
              "rescue_on_R", "rescue_round2", "containment_removals", "fourth_not_rescued", "num_output_cuts", "full_cut"):
        assert shown[k] >= 1, k
    v = shown["tie_winner_by_vscore"]
    assert v == [7, 8, 7, 5], v          # (a spoiled segment gives 5 votes, 8 clean seeds 7, 9 clean seeds 8: which segment won shows in vscore)
    out = {"read_%d" % i: r for i, r in enumerate(reads)}
    out["cases"] = np.array(json.dumps(meta))
    record_tool(tmp, base, XC.ref_codes(base["ref_fasta"].tobytes())[0], out, shown)
    print(shown["tool"], file=sys.stderr)
    out["asserted"] = np.array(json.dumps(shown))
    np.savez_compressed(SC.FIXTURE + ".new.npz", **out)
    os.replace(SC.FIXTURE + ".new.npz", SC.FIXTURE)
    shutil.rmtree(tmp, ignore_errors=True)
    print("bytes", os.path.getsize(SC.FIXTURE), file=sys.stderr)


if __name__ == "__main__":
    main()
