#!/usr/bin/env python3
"""What the FASTA text on the device costs against the host pass it replaces, and the first end-to-end figure of the mecat2cns program.
Config 4's batch (every template of config 2's own overlaps, as tools/cns_reads_time.py builds it; its first 10 000 templates by
default) through two call shapes:

    (a) mhip_cns_correct_templates     TEXT     the accepted records and the text cross the link
    (b) mhip_cns_accept_templates_reads READS   followed by mhip_cns_format_reads on the host: the parent commit's way

one warm-up per shape, then `--passes` timed passes per shape, alternating, context profiling on so that the cns_text_* kernels appear in
the kernel statistics.  Wall time is taken around the calls of the Python binding, a device-wide wait on either side.

Then the program: mecat_amd/bin/mecat2cns -i 0 on the `.can` lines that touch those templates (every candidate line with one of its
reads among them; the partition step makes a template of the other read as well, most of which the coverage gate drops) and the whole
read set as FASTA, once with the device text and once with MECAT_CNS_HOST_TEXT=1, each a child process under its own time limit.
Corrected bases per second = letters of the output's records / the process's wall time, the reading of the 1.5 GB FASTA included.

    python tools/cns_cli_time.py [--templates N] [--passes K] [--out FILE] [--no-driver]

Writes a small markdown report (default profiles/cns_cli.md).  Measures; asserts only that the texts of (a) and (b) are equal and that
the program's two outputs are."""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT_KERNELS = ("cns_text_size", "cns_text_scan", "cns_text_write")


def spread(x):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(x)), min(x), max(x)) if len(x) else "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--templates", type=int, default=10000, help="first N templates only (0: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cns_cli.md"))
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--no-driver", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (its HIP runtime first, as in the tests)
    from mecat_amd import hip as M, workload as W

    n, L, err, G, seed, ont = W.CONFIGS["config2"]
    t0 = time.time()
    codes, lens = W.synth_reads(n, L, err, G, seed, ont)
    pac, offs, num_bases = W.pack_volume(codes, lens)
    ctx = M.Context(0)
    vol = M.Volume(ctx, pac, offs, num_bases, 0)
    params = M.default_params(ont)
    idx = M.Index(ctx, vol)
    cands, cnt = M.seed_reads(ctx, idx, vol, vol, 0, n, params)
    idx.free()
    ec = W.ext_candidates_from_table(cands, cnt, lens)
    min_cov, min_size, mas, ratio = 6, 5000, 2000, 0.9          # mecat2cns' PacBio defaults
    rec, tb, ids = W.cns_templates(ec, n, min_cov, min_size)
    del cands
    T = len(ids) if args.templates <= 0 else min(len(ids), args.templates)
    rec = np.ascontiguousarray(rec[: tb[T]])
    tb = tb[: T + 1]
    threads = int(os.environ.get("MECAT_BENCH_THREADS", 16))
    print("[cns_cli_time] %d templates, %d records, set up in %.1f s" % (T, len(rec), time.time() - t0), file=sys.stderr, flush=True)

    def call_a():
        ctx.sync()
        c0 = time.perf_counter()
        out, text, _, _ = M.cns_correct_templates(ctx, vol, rec, tb, ont, mas, ratio, M.CNS_WANT_TEXT, min_cov, min_size, threads=threads)
        ctx.sync()
        return time.perf_counter() - c0, text, len(out[0]) * M.ACCEPTED_DTYPE.itemsize + len(text)

    def call_b():
        r = rec.copy()
        ctx.sync()
        c0 = time.perf_counter()
        out = M.cns_accept_templates_reads(ctx, vol, r, tb, ont, mas, ratio, M.CNS_WANT_READS, min_cov, min_size, threads=threads)
        rd = out[7]
        text = M.cns_format_reads(rd["reads"], rd["seq"])
        ctx.sync()
        return time.perf_counter() - c0, text, len(out[0]) * M.ACCEPTED_DTYPE.itemsize + rd["reads"].nbytes + rd["seq"].nbytes + rd["read_begin"].nbytes

    ctx.set_profiling(True)
    walls, moved, kms, texts = {"a": [], "b": []}, {}, {k: [] for k in TEXT_KERNELS}, {}
    for f in (call_a, call_b):
        f()
    for _ in range(args.passes):
        for key, f in (("a", call_a), ("b", call_b)):
            ctx.reset_stats()
            dt, text, nbytes = f()
            walls[key].append(dt)
            moved[key] = nbytes
            texts[key] = hashlib.sha256(text).hexdigest()
            if key == "a":
                st = ctx.kernel_stats()
                for k in TEXT_KERNELS:
                    kms[k].append(st.get(k, (0, 0.0))[1])
                nrec, nbases = text.count(b">"), len(text)
    ctx.set_profiling(False)
    assert texts["a"] == texts["b"], "the device text and the host text differ"
    vol.free()
    ctx.close()

    a, b = walls["a"], walls["b"]
    diff = float(np.median(a) - np.median(b))
    width = max(max(a) - min(a), max(b) - min(b))
    slower = diff > width
    lines = ["# The FASTA text on the device, and the mecat2cns program end to end", "",
             "`python tools/cns_cli_time.py` on one MI355X: the first %d templates of config 4's batch (%d candidate records), %d host threads, min_cov %d / min_size %d.  One warm-up "
             "per call shape, then %d timed passes per shape, alternating; context profiling on; wall time around the calls of the Python binding.  Median (min .. max)." %
             (T, len(rec), threads, min_cov, min_size, args.passes), "",
             "The text: %d records, %d bytes; the two shapes' texts are equal byte for byte (SHA-256 %s)." % (nrec, nbases, texts["a"][:16]), "",
             "| call shape | wall per pass (s) | bytes over the link towards the host |", "|---|---|---|",
             "| (a) `mhip_cns_correct_templates`, TEXT | %s | %d |" % (spread(a), moved["a"]),
             "| (b) `mhip_cns_accept_templates_reads`, READS + `mhip_cns_format_reads` | %s | %d |" % (spread(b), moved["b"]), "",
             "Text kernels, ms per pass of (a): " + ", ".join("`%s` %s" % (k, spread(kms[k])) for k in TEXT_KERNELS) + ".", "",
             "Kernel resources (`-Rpass-analysis=kernel-resource-usage`, gfx950): `cns_text_size` 14 VGPRs, `cns_text_scan` 62, `cns_text_write` 36; no scratch in any of them; "
             "`cns_text_write`'s copy loop is `global_load_dwordx4` x 2, four `v_alignbyte_b32`, `global_store_dwordx4`.", "",
             "Decision: (a) - (b) = %+.3f s between the medians; the passes of a shape spread over %.3f s.  The device text is %s the host text beyond the spread, so the "
             "program's default is the **%s** text." % (diff, width, "slower than" if slower else "not slower than", "host" if slower else "device"), ""]

    if not args.no_driver:
        exe = os.path.join(ROOT, "mecat_amd", "bin", "mecat2cns")
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "reads.fasta")
            W.write_fasta(fa, codes, lens)
            chosen = np.zeros(n, bool)
            chosen[ids[:T]] = True
            sel = ec[chosen[ec[:, 1]] | chosen[ec[:, 7]]]
            can = os.path.join(d, "cands.can")
            # a `.can` line: qid sid qdir sdir qext sext score qsize ssize (common/alignment.cpp:18-32)
            np.savetxt(can, sel[:, [1, 7, 0, 6, 2, 8, 12, 3, 9]], fmt="%d", delimiter="\t")
            rows, shas = [], []
            for label, env in (("device text", {}), ("host text (`MECAT_CNS_HOST_TEXT=1`)", {"MECAT_CNS_HOST_TEXT": "1"})):
                out = os.path.join(d, "out.fasta")
                c0 = time.perf_counter()
                r = subprocess.run([exe, "-i", "0", "-t", str(threads), can, fa, out], env=dict(os.environ, **env), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
                dt = time.perf_counter() - c0
                assert r.returncode == 0, r.stderr.decode()[-2000:]
                text = open(out, "rb").read()
                bases = sum(len(l) for l in text.split(b"\n")[1::2])
                shas.append(hashlib.sha256(text).hexdigest())
                rows.append("| %s | %.2f | %d | %d | %.3e |" % (label, dt, text.count(b">"), bases, bases / dt))
            assert shas[0] == shas[1], "the program's two outputs differ"
        lines += ["## The program", "",
                  "`mecat2cns -i 0 -t %d` (PacBio defaults) on the %d `.can` lines that touch those templates and the whole read set (%d reads, %.2f Gbase) as one FASTA file; one "
                  "run each, a fresh process, wall time of the process: the partition step, reading the FASTA, the upload, the partitions, the output file.  The two outputs are "
                  "equal byte for byte.  **This is the drop-in's figure alone**: the compiled reference program is not part of the test set-up, so there is no reference time beside it." %
                  (threads, len(sel), n, float(lens.astype(np.int64).sum()) / 1e9), "",
                  "| text | wall (s) | records | corrected bases | corrected bases per second |", "|---|---|---|---|---|"] + rows + [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
