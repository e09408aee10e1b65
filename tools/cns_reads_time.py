#!/usr/bin/env python3
"""What assembling the corrected reads on the device costs in the accept stage: config 4's batch (every template of config 2's own
overlaps, as tools/cns_poa_time.py builds it; its first 10 000 templates by default) through

    parent commit's library   mhip_cns_accept_templates_poa    PLAN | POA           (--parent-tree DIR, a child process of this tool)
    this library              mhip_cns_accept_templates_reads  PLAN | POA           the call without the bit: must cost what the parent's costs
    this library              mhip_cns_accept_templates_reads  PLAN | POA | READS   plan, consensus and reads
    this library              mhip_cns_accept_templates_reads  READS                the accepted records and the reads, nothing else

one warm-up per mode, then `--passes` timed passes per mode, the modes ALTERNATING pass by pass, with context profiling on so that the
cns_reads_* kernels appear in the kernel statistics (HIP events around every launch) and MECAT_CNS_TIMES=1, whose stderr lines give the
host waits.  Wall time is taken around the call of the Python binding, a device-wide wait on either side.  The parent's passes are
measured by a child process in the same session, started once this process has freed its volume and closed its context, with the
parent's own mecat_amd package (`make hip synth` in a checkout of the parent commit).

    python tools/cns_reads_time.py [--templates N] [--passes K] [--parent-tree DIR] [--out FILE]

Writes a small markdown report (default profiles/cns_reads.md).  Measures; asserts only that the reads of the two modes with the bit are
equal."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ_KERNELS = ("cns_reads_size", "cns_reads_scan", "cns_reads_records", "cns_reads_letters")
POA_KERNELS = ("cns_poa_bound", "cns_poa_scan", "cns_poa_small", "cns_poa_list", "cns_poa_large", "cns_poa_widen", "cns_poa_gather")


def spread(x):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(x)), min(x), max(x)) if len(x) else "-"


def moved(out):
    """bytes of a call's outputs (what crossed the link towards the host)"""
    n = sum(int(np.asarray(x).nbytes) for x in (out[0], out[1], out[3], out[4], out[5]))
    for d in out[6:]:
        if isinstance(d, dict):
            n += sum(int(v.nbytes) for v in d.values())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--templates", type=int, default=10000, help="first N templates only (0: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cns_reads.md"))
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: its `_poa` PLAN | POA passes, from a child process")
    ap.add_argument("--poa-only-json", action="store_true", help="(the child) mhip_cns_accept_templates_poa, PLAN | POA passes only, one JSON line on stdout")
    ap.add_argument("--tree", default=ROOT, help="(the child) where mecat_amd is imported from")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    os.environ["MECAT_CNS_TIMES"] = "1"          # the call's own breakdown on stderr
    import torch  # noqa: F401  (its HIP runtime first, as in the tests)
    from mecat_amd import hip as M, workload as W

    n, L, err, G, seed, ont = W.CONFIGS["config2"]
    t0 = time.time()
    codes, lens = W.synth_reads(n, L, err, G, seed, ont)
    pac, offs, num_bases = W.pack_volume(codes, lens)
    del codes
    ctx = M.Context(0)
    vol = M.Volume(ctx, pac, offs, num_bases, 0)
    params = M.default_params(ont)
    idx = M.Index(ctx, vol)
    cands, cnt = M.seed_reads(ctx, idx, vol, vol, 0, n, params)
    idx.free()
    ec = W.ext_candidates_from_table(cands, cnt, lens)
    rec, tb, ids = W.cns_templates(ec, n)
    del cands, ec
    T = len(ids) if args.templates <= 0 else min(len(ids), args.templates)
    rec = np.ascontiguousarray(rec[: tb[T]])
    tb = tb[: T + 1]
    tbases = int(lens[ids[:T]].astype(np.int64).sum())
    threads = int(os.environ.get("MECAT_BENCH_THREADS", min(64, os.cpu_count() or 1)))
    print("[cns_reads_time] %d templates, %d records, %.2f Gbase of templates, set up in %.1f s" % (T, len(rec), tbases / 1e9, time.time() - t0), file=sys.stderr, flush=True)
    mas, ratio = (params.min_align_size if ont else 2000), (0.4 if ont else 0.9)
    min_cov, min_size = (6, 2000) if ont else (4, 5000)          # mecat2cns' defaults
    PL, PO = 4, 16
    RD = 0 if args.poa_only_json else M.CNS_WANT_READS

    def call(mode):
        r = rec.copy()
        ctx.sync()
        sys.stderr.flush()
        keep = os.dup(2)
        with tempfile.TemporaryFile() as tmp:       # the library's stderr lines of this call
            os.dup2(tmp.fileno(), 2)
            try:
                c0 = time.perf_counter()
                f = M.cns_accept_templates_poa if args.poa_only_json else M.cns_accept_templates_reads
                out = f(ctx, vol, r, tb, ont, mas, ratio, mode, min_cov, min_size, threads=threads)
                ctx.sync()
                dt = time.perf_counter() - c0
            finally:
                os.dup2(keep, 2)
                os.close(keep)
            tmp.seek(0)
            text = tmp.read().decode(errors="replace")
        sys.stderr.write(text)
        return dt, out, text

    if args.poa_only_json:
        modes = [("`_poa`, PLAN \\| POA", PL | PO)]
    else:
        modes = [("`_reads`, PLAN \\| POA", PL | PO), ("`_reads`, PLAN \\| POA \\| READS", PL | PO | RD), ("`_reads`, READS", RD)]
    ctx.set_profiling(True)
    walls = {m: [] for _, m in modes}
    kms = {m: {} for _, m in modes}
    host = {m: dict(wait=[], rwait=[], slices=[]) for _, m in modes}      # from the library's stderr lines
    nbytes, reads, nacc, plan = {}, {}, 0, None
    for _, m in modes:
        call(m)                                     # warm-up: scratch buffers, result buffers, page locking
    for _ in range(args.passes):
        for _, m in modes:                          # alternating: a drift of the host hits every mode alike
            ctx.reset_stats()
            dt, out, text = call(m)
            walls[m].append(dt)
            for key, pat in (("wait", r"waited for the counts ([0-9.]+)"), ("rwait", r"waited for the totals ([0-9.]+)"), ("slices", r"jobs in (\d+) slices")):
                f = re.search(pat, text)
                if f:
                    host[m][key].append(float(f.group(1)))
            for k, (launches, ms) in ctx.kernel_stats().items():
                kms[m].setdefault(k, []).append(ms)
            nbytes[m] = moved(out)
            nacc = len(out[0])
            if len(out) > 7 and out[7] is not None:
                reads[m] = {k: np.array(v, copy=True) for k, v in out[7].items()}
            if out[6] is not None:
                plan = dict(segments=len(out[6]["segments"]), windows=len(out[6]["windows"]), cns=len(out[6]["cns"]))
            del out
    ctx.set_profiling(False)
    vol.free()
    ctx.close()
    if args.poa_only_json:
        print(json.dumps(dict(walls=walls[PL | PO], templates=T)))
        return
    a, b = reads[PL | PO | RD], reads[RD]
    same = all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert same, "the reads of PLAN | POA | READS and of READS alone differ"

    parent = None
    if args.parent_tree:
        cmd = [sys.executable, os.path.abspath(__file__), "--poa-only-json", "--tree", os.path.abspath(args.parent_tree), "--passes", str(args.passes),
               "--templates", str(args.templates)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=1500, check=True)
        parent = json.loads(r.stdout.decode().strip().splitlines()[-1])

    full = PL | PO | RD
    rk = {k: kms[full].get(k, [0.0]) for k in READ_KERNELS}
    per_pass = [sum(rk[k][i] if i < len(rk[k]) else 0.0 for k in READ_KERNELS) for i in range(args.passes)]
    poa_ms = sum(float(np.median(kms[full].get(k, [0.0]))) for k in POA_KERNELS)
    nr, nl = len(a["reads"]), len(a["seq"])
    cut = int((np.diff(np.concatenate([a["reads"]["segment"], [-1]])) == 0).sum())
    lines = ["# The corrected reads assembled on the device behind the POA: what the stage costs", "",
             "`python tools/cns_reads_time.py` on one MI355X: the first %d templates of config 4's batch (%.2f Gbase of templates, %d candidate records, %d accepted alignments), "
             "%d host threads, min_cov %d / min_size %d.  One warm-up per mode, then %d timed passes per mode, the modes alternating pass by pass; context profiling on (HIP "
             "events around every kernel launch); wall time around the call of the Python binding.  Median (min .. max) over the passes." %
             (T, tbases / 1e9, len(rec), nacc, threads, min_cov, min_size, args.passes), "",
             "The plan: %d segments, %d windows, %d bytes of window consensus.  The reads: **%d records, %d letters** (%d records belong to segments that were cut into "
             "overlapping blocks); the reads of `PLAN | POA | READS` and of `READS` alone are equal byte for byte: %s." %
             (plan["segments"], plan["windows"], plan["cns"], nr, nl, cut, same), "",
             "| call | wall per pass (s) | host waits: plan + pieces + POA + reads (s) | of which the reads' wait (s) | bytes the call hands over |", "|---|---|---|---|---|"]
    if parent:
        lines.append("| parent commit's library, `_poa`, PLAN \\| POA (child process, same session) | %s | | | |" % spread(parent["walls"]))
    for label, m in modes:
        lines.append("| %s | %s | %s | %s | %d |" % (label, spread(walls[m]), spread(host[m]["wait"]), spread(host[m]["rwait"]), nbytes[m]))
    lines += ["", "The batch ran in %d slices; with `READS` every slice waits once more, for the two totals (letters, records) that size the output — the third column's share "
              "of the second.  The wait is a stream synchronisation behind `cns_poa_gather`, `cns_reads_size` and `cns_reads_scan`, so the figure in the third column is mostly "
              "the POA kernels still running when the host gets there — time the host otherwise spends in the wait for the last copies.  It moves a wait, it does not add "
              "one of that length: what the stage adds to a call is the difference of the wall times below." % (int(host[full]["slices"][0]) if host[full]["slices"] else 0), "",
              "Bytes: the accepted records come with every mode; `PLAN | POA` adds segments, windows, effective ranges and the windows' consensus with its begin array; `READS` "
              "alone adds only the read records, their letters and one begin entry per template.", ""]
    if parent:
        p, q = parent["walls"], walls[PL | PO]
        lines += ["Requirement — `_reads` without the bit costs what the parent's `_poa` costs in the same mode, within the spread of the passes of the two: parent %s s, this "
                  "library %s s; the medians differ by %+.3f s, the passes of either spread over %.3f s and %.3f s." %
                  (spread(p), spread(q), float(np.median(q) - np.median(p)), max(p) - min(p), max(q) - min(q)), ""]
    lines += ["`READS` against `PLAN | POA` (this library): `PLAN | POA | READS` %+.3f s, `READS` alone %+.3f s (differences of the medians)." %
              (float(np.median(walls[full]) - np.median(walls[PL | PO])), float(np.median(walls[RD]) - np.median(walls[PL | PO]))), "",
              "Read kernels, ms per pass (PLAN | POA | READS), all launches of a pass summed:", "", "| " + " | ".join("`%s`" % k for k in READ_KERNELS) + " | all |",
              "|" + "---|" * (len(READ_KERNELS) + 1), "| " + " | ".join(spread(rk[k]) for k in READ_KERNELS) + " | **%s** |" % spread(per_pass), "",
              "The POA kernels in the same passes: %.2f ms." % poa_ms, ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
