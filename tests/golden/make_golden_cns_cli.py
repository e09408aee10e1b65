#!/usr/bin/env python3
"""Golden vectors for the mecat2cns program (mecat_amd/cns/cns_main.cpp) and the m4 walk of its accept stage: the UNMODIFIED mecat2cns
(oracle/_ref/libref_cns_accept.so = all of it except main.cpp) behind cns_cli_ref_main.cpp next to this file, compiled into a temporary
directory against the reference's headers where they lie, on overlap files written by the UNMODIFIED oracle/_ref/mecat2pw.  Build
container only:
    python tests/golden/make_golden_cns_cli.py
Writes tests/golden/cns_cli.npz, data only: the read sets as generator parameters (H.synth_reads), the `.can` and `-j 1 -g 1` `.m4`
text of the reference overlapper as compressed bytes (both programs read the same file), the options of the four recorded runs
(technology x input type), per run SHA-256 of the whole output, every header line, SHA-256 of every record and the first 8 records in
full; per m4 run and template what consensus_one_read_m4_* accepted — (soff, send, aln_size) in order and a SHA-256 over the normalised
strings —, its cns_results, and per record the walk looked at the result of GetAlignment on it (a second call by the harness); and stdout, stderr and exit code of the command line on the argv vectors of CLI_VECTORS.  The script
asserts, on the reference alone, what the fixture must show (the end of main) and stores the counts."""
import hashlib
import json
import lzma
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cns_poa_cases as P  # noqa: E402
import helpers as H  # noqa: E402

REF_ROOT = P.REF_ROOT
REF_LIB = os.path.join(H.ROOT, "oracle", "_ref", "libref_cns_accept.so")
REF_PW = os.path.join(H.ROOT, "oracle", "_ref", "mecat2pw")
FIXTURE = os.path.join(H.GOLDEN, "cns_cli.npz")

# name: read set (nreads, L, err, genome, seed, ont: cns_accept.npz's two sets), tech, and the run's options: -p gives 3 partitions, -k
# fewer files than partitions (the multi-pass partitioning runs), -a large enough that GetAlignment refuses the shorter overlaps (it
# counts alignment columns, gaps included) — for nanopore 2 150 columns, where alignments of about 1 900 bases fall on either side: some
# fail, some succeed and are then refused by the mapping range's 0.48 * read length —, -l so
# that the sets produce reads.  PacBio's -c 28 lies above the smallest templates' record counts (26 and 27 in the m4 partitions), so the
# driver's coverage gate drops templates.  Its size gate (ssize < 0.95 * min_size) cannot fire in a whole run: the partition step has
# already dropped every line with a read shorter than min_size (overlaps_partition.cpp) — tests/test_cns_cli_cpu.py feeds it by hand.
SETS = {
    "pacbio": dict(reads=(240, 5000, 0.15, 12000, 77, 0), tech=0, opts={"-p": "80", "-k": "2", "-a": "4000", "-r": "0.6", "-c": "28", "-l": "3000"}),
    "nanopore": dict(reads=(160, 4000, 0.12, 8000, 78, 1), tech=1, opts={"-p": "60", "-k": "2", "-a": "2150", "-r": "0.5", "-c": "4", "-l": "3000"}),
}
MAX_ADDED = {0: 60, 1: 100}

CLI_VECTORS = [
    ["-h", "a", "b", "c"],                                   # the defaults of PacBio
    ["-x", "1", "-h", "a", "b", "c"],                        # the defaults of nanopore
    ["-x", "0", "-i", "0", "-t", "3", "-p", "7", "-r", "0.25", "-a", "9", "-c", "2", "-l", "11", "-k", "5", "-h", "a", "b", "c"],
    ["-t", "0", "a", "b", "c"],
    ["-p", "0", "a", "b", "c"],
    ["-r", "-0.5", "a", "b", "c"],
    ["-c", "-1", "a", "b", "c"],                             # both messages of the min_cov test
    ["-t", "-2", "-p", "-3", "-r", "-1", "-c", "-4", "a", "b", "c"],
    ["-i", "2", "a", "b", "c"],
    ["-z", "a", "b", "c"],                                   # an unknown option
    ["a", "b", "c", "-c"],                                   # a missing argument
    ["-h"],                                                  # fewer than three words in all
    [],
    ["a"],
]


def build_ref_program(tmp):
    exe = os.path.join(tmp, "cns_cli_ref")
    src = os.path.join(REF_ROOT, "src")
    subprocess.run(["g++", "-O2", "-w", "-pthread", "-fopenmp", "-I" + src, "-I" + os.path.join(src, "mecat2cns"), "-I" + os.path.join(src, "mecat2cns", "libboost"),
                    os.path.join(H.GOLDEN, "cns_cli_ref_main.cpp"), REF_LIB, "-Wl,-rpath," + os.path.dirname(REF_LIB), "-o", exe], check=True)
    return exe


def overlapper(fa, tmp, task, tech):
    out = os.path.join(tmp, "ov%d" % task)
    wrk = os.path.join(tmp, "w%d" % task)
    subprocess.run([REF_PW, "-j", str(task), "-d", fa, "-o", out, "-w", wrk, "-t", "8", "-g", "1", "-x", str(tech)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out, "rb").read()


def packed(a):
    """an int32 table as LZMA bytes of its columns one behind the other (a third smaller than the .npz's deflate of the rows): read back
    by tests/cns_cli_cases.py table()"""
    a = np.ascontiguousarray(a, dtype=np.int32)
    return np.frombuffer(lzma.compress(np.ascontiguousarray(a.T).tobytes(), preset=9 | lzma.PRESET_EXTREME), dtype=np.uint8)


def records_of(text):
    """the output file -> [(header line, letters)]"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    return [(lines[i], lines[i + 1]) for i in range(0, len(lines) - 1, 2)]


def parse_walk(data):
    """cns_cli_ref_main m4walk's file -> ([template dict], drop_cov, drop_size)"""
    p, out = 0, []

    def ints(n):
        nonlocal p
        v = struct.unpack_from("<%di" % n, data, p)
        p += 4 * n
        return v
    while True:
        sid, = ints(1)
        if sid == -1:
            drop_cov, drop_size = ints(2)
            assert p == len(data)
            return out, drop_cov, drop_size
        nrec, looked, aligned, refused = ints(4)
        seen = [ints(7) for _ in range(looked)]
        nal, = ints(1)
        meta, sha = [], hashlib.sha256()
        for _ in range(nal):
            soff, send, n = ints(3)
            meta.append((soff, send, n))
            sha.update(data[p: p + 2 * (n + 1)])
            p += 2 * (n + 1)
        nres, = ints(1)
        res = []
        for _ in range(nres):
            rid, r0, r1, n = ints(4)
            res.append((rid, r0, r1, n, hashlib.sha256(data[p: p + n]).hexdigest()))
            p += n
        out.append(dict(sid=sid, nrec=nrec, looked=looked, aligned=aligned, refused=refused, seen=seen, meta=meta, sha=sha.hexdigest(), results=res))


def main():
    out, asserted = {}, {}
    tmp = tempfile.mkdtemp(prefix="cnscli_")
    exe = build_ref_program(tmp)
    # ---- the command line
    cli = []
    for argv in CLI_VECTORS:
        r = subprocess.run([exe, "cli"] + argv, capture_output=True, cwd=tmp)
        cli.append(dict(argv=argv, stdout=r.stdout.decode(), stderr=r.stderr.decode(), rc=r.returncode))
        assert r.returncode in (0, 1), (argv, r.returncode)
    out["cli"] = np.array(json.dumps(cli))
    # ---- the runs
    for name, S in SETS.items():
        tech = S["tech"]
        codes, lens = H.synth_reads(*S["reads"])
        fa = os.path.join(tmp, name + ".fa")
        H.write_fasta(fa, codes, lens)
        os.makedirs(os.path.join(tmp, name))
        texts = [overlapper(fa, os.path.join(tmp, name), task, tech) for task in (0, 1)]
        out[name + "_reads"] = np.array(S["reads"][:2] + S["reads"][3:], dtype=np.int64)
        out[name + "_err"] = np.array([S["reads"][2]])
        out[name + "_opts"] = np.array(json.dumps(S["opts"]))
        for it in (0, 1):
            key = "%s_%s" % (name, ("can", "m4")[it])
            out[key + "_input"] = np.frombuffer(lzma.compress(texts[it], preset=9 | lzma.PRESET_EXTREME), dtype=np.uint8)
            rd = os.path.join(tmp, key)
            os.makedirs(rd)
            inp = os.path.join(rd, "ov")
            open(inp, "wb").write(texts[it])
            res = os.path.join(rd, "out.fasta")
            argv = ["-x", str(tech), "-i", str(it), "-t", "1"] + [x for kv in S["opts"].items() for x in kv] + [inp, fa, res]
            subprocess.run([exe, "cli"] + argv, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            text = open(res, "rb").read()
            recs = records_of(text)
            parts = [l.split("\t") for l in open(inp + ".partition_files").read().splitlines()]
            out[key + "_sha"] = np.array(hashlib.sha256(text).hexdigest())
            out[key + "_headers"] = np.array([h.decode() for h, _ in recs])
            out[key + "_record_sha"] = np.array([hashlib.sha256(h + b"\n" + s + b"\n").hexdigest() for h, s in recs])
            out[key + "_first"] = np.array(b"".join(h + b"\n" + s + b"\n" for h, s in recs[:8]).decode())
            count = dict(records=len(recs), partitions=len(parts), bytes=len(text), lines=texts[it].count(b"\n"))
            if it == 1:
                drops, walk = [0, 0], []
                for pf, _, _ in parts:
                    wf = os.path.join(rd, "walk.bin")
                    subprocess.run([exe, "m4walk", pf, fa, str(tech), S["opts"]["-a"], S["opts"]["-r"], S["opts"]["-c"], S["opts"]["-l"], wf], check=True,
                                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                    w, dc, ds = parse_walk(open(wf, "rb").read())
                    walk += w
                    drops[0] += dc
                    drops[1] += ds
                # the walk's results are the run's records
                flat = [r for t in walk for r in t["results"]]
                assert [b">%d_%d_%d_%d" % r[:4] for r in flat] == [h for h, _ in recs], key
                assert [r[4] for r in flat] == [hashlib.sha256(s).hexdigest() for _, s in recs], key
                out[key + "_walk_sid"] = np.array([t["sid"] for t in walk], dtype=np.int32)
                out[key + "_walk_counts"] = np.array([[t["nrec"], t["looked"], t["aligned"], t["refused"], len(t["meta"]), len(t["results"])] for t in walk], dtype=np.int32)
                # per record the walk looked at: ok, qoff, qend, soff, send of its alignment, qsize, ssize (int16 planes would not hold them)
                out[key + "_walk_seen"] = packed(np.array([r for t in walk for r in t["seen"]], dtype=np.int32).reshape(-1, 7))
                out[key + "_walk_meta"] = packed(np.array([m for t in walk for m in t["meta"]], dtype=np.int32).reshape(-1, 3))
                out[key + "_walk_sha"] = np.array([t["sha"] for t in walk])
                out[key + "_walk_results"] = np.array([r[:4] for r in flat], dtype=np.int32).reshape(-1, 4)
                out[key + "_walk_result_sha"] = np.array([r[4] for r in flat])
                nrec = np.array([t["nrec"] for t in walk])
                count.update(templates=len(walk), drop_cov=drops[0], drop_size=drops[1], over_max=int((nrec > MAX_ADDED[tech]).sum()), upto_max=int((nrec <= MAX_ADDED[tech]).sum()),
                             align_failed=int(sum(t["looked"] - t["aligned"] for t in walk)), ratio_refused=int(sum(t["refused"] for t in walk)),
                             accepted=int(sum(len(t["meta"]) for t in walk)))
                assert all(len(t["meta"]) == t["aligned"] - (t["refused"] if tech == 1 else 0) for t in walk), key
            asserted[key] = count
            print(key, count, file=sys.stderr)
    # ---- what the fixture must show (on the reference alone)
    for key, c in asserted.items():
        assert c["records"] >= 20 and c["partitions"] >= 3, (key, c)
    for name in SETS:
        m4 = asserted[name + "_m4"]
        assert m4["over_max"] >= 1 and m4["upto_max"] >= 1 and m4["align_failed"] >= 1, (name, m4)
    assert asserted["nanopore_m4"]["ratio_refused"] >= 1
    assert any(asserted[n + "_m4"]["drop_cov"] >= 1 for n in SETS)
    assert all(asserted[n + "_m4"]["drop_size"] == 0 for n in SETS)          # (unreachable behind the partition step: see SETS)
    out["asserted"] = np.array(json.dumps(asserted))
    np.savez_compressed(FIXTURE + ".new.npz", **out)
    os.replace(FIXTURE + ".new.npz", FIXTURE)
    shutil.rmtree(tmp, ignore_errors=True)
    print("bytes", os.path.getsize(FIXTURE), file=sys.stderr)


if __name__ == "__main__":
    main()
