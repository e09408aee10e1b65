#!/usr/bin/env python3
"""What the consensus plan costs in the accept stage: config 4's batch (every template of config 2's own overlaps, as
tools/cns_table_time.py and bench.py --workload config4 build it) through

    mhip_cns_accept_templates_ex    TABLE           the tables alone, as before
    mhip_cns_accept_templates_plan  TABLE | PLAN    tables and plan
                                    PLAN            the plan alone: neither strings nor tables cross the PCIe link

one warm-up each, then `--passes` timed passes per mode, the modes ALTERNATING pass by pass (other work shares the host), with context
profiling on so that cns_plan_segments / cns_plan_count / cns_plan_emit (and scan, compact, cns_table_finish) appear in the kernel
statistics — HIP events around every launch — and MECAT_CNS_TIMES=1, whose stderr lines say how long the host waited for the plan's
counts and how long it took to put the slices' pieces together.  --parent-tree DIR: a checkout of the parent commit with its library
built (`make hip synth`); its TABLE pass is measured by a child process of this tool in the same session, started once this process has
freed its volume and closed its context (two processes have the GPU open meanwhile), with the parent's own mecat_amd package, and set
next to the others.  Wall time is taken around the call of the Python binding, a device-wide wait on either side.
Writes a small markdown report (default profiles/cns_plan.md).  Measures; asserts only that the plans of the two PLAN modes are equal.

    python tools/cns_plan_time.py [--templates N] [--passes K] [--parent-tree DIR] [--out FILE]
"""
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
FINISH_MS_EXPECTED = 19.0       # cns_table_finish per pass in profiles/cns_table.md: what the plan was expected to cost, about
PLAN_KERNELS = ("cns_plan_segments", "cns_plan_scan", "cns_plan_compact", "cns_plan_count", "cns_plan_emit")


def spread(x):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(x)), min(x), max(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--templates", type=int, default=0, help="first N templates only (0: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cns_plan.md"))
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: its TABLE pass, from a child process")
    ap.add_argument("--table-only-json", action="store_true", help="(the child) TABLE passes only, one JSON line on stdout")
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
    print("[cns_plan_time] %d templates, %d records, %.2f Gbase of templates, set up in %.1f s" % (T, len(rec), tbases / 1e9, time.time() - t0), file=sys.stderr, flush=True)
    mas, ratio = (params.min_align_size if ont else 2000), (0.4 if ont else 0.9)
    min_cov, min_size = (6, 2000) if ont else (4, 5000)          # mecat2cns' defaults

    def call(mode):
        r = rec.copy()
        ctx.sync()
        sys.stderr.flush()
        keep = os.dup(2)
        with tempfile.TemporaryFile() as tmp:       # the library's stderr lines of this call
            os.dup2(tmp.fileno(), 2)
            try:
                c0 = time.perf_counter()
                if mode & 4:
                    out = M.cns_accept_templates_plan(ctx, vol, r, tb, ont, mas, ratio, mode, min_cov, min_size, threads=threads)
                else:
                    out = M.cns_accept_templates_ex(ctx, vol, r, tb, ont, mas, ratio, mode, threads=threads) + (None,)
                ctx.sync()
                dt = time.perf_counter() - c0
            finally:
                os.dup2(keep, 2)
                os.close(keep)
            tmp.seek(0)
            text = tmp.read().decode(errors="replace")
        sys.stderr.write(text)
        return dt, out, text

    modes = [("_ex, TABLE", 2)] if args.table_only_json else [("_ex, TABLE", 2), ("_plan, TABLE \\| PLAN", 6), ("_plan, PLAN", 4)]
    ctx.set_profiling(True)
    walls = {m: [] for _, m in modes}
    kms = {m: {} for _, m in modes}
    plans, shape = {}, {}
    host = {m: dict(wait=[], put=[], slices=[]) for _, m in modes}      # from the library's stderr lines
    for _, m in modes:
        call(m)                                     # warm-up: scratch buffers, result buffers, page locking
    for _ in range(args.passes):
        for _, m in modes:                          # alternating: a drift of the host hits every mode alike
            ctx.reset_stats()
            dt, out, text = call(m)
            walls[m].append(dt)
            for key, pat in (("wait", r"waited for the counts ([0-9.]+)"), ("put", r"put together ([0-9.]+)"), ("slices", r"jobs in (\d+) slices")):
                f = re.search(pat, text)
                if f:
                    host[m][key].append(float(f.group(1)))
            for k, (launches, ms) in ctx.kernel_stats().items():
                kms[m].setdefault(k, []).append(ms)
            if out[6] is not None:
                plans[m] = out[6]
            shape[m] = (len(out[0]), len(out[3]))
            del out
    ctx.set_profiling(False)
    vol.free()
    ctx.close()
    if args.table_only_json:
        print(json.dumps(dict(walls=walls[2], finish_ms=kms[2].get("cns_table_finish", []), templates=T)))
        return
    same = all(plans[6][k].tobytes() == plans[4][k].tobytes() for k in plans[6])
    assert same, "the plans of TABLE | PLAN and PLAN differ"
    p = plans[4]
    positions = int((p["segments"]["end"].astype(np.int64) - p["segments"]["beg"]).sum())

    parent = None
    if args.parent_tree:
        cmd = [sys.executable, os.path.abspath(__file__), "--table-only-json", "--tree", os.path.abspath(args.parent_tree), "--passes", str(args.passes),
               "--templates", str(args.templates)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=1500, check=True)
        parent = json.loads(r.stdout.decode().strip().splitlines()[-1])

    med = lambda m, k: float(np.median(kms[m].get(k, [0.0])))
    plan_ms = sum(med(6, k) for k in PLAN_KERNELS)
    lines = ["# The consensus plan in the accept stage: what it costs", "",
             "`python tools/cns_plan_time.py%s` on one MI355X: config 4's batch (%d templates of config 2's overlaps, %.2f Gbase of templates = table positions, %d candidate "
             "records, %d accepted alignments), %d host threads, min_cov %d / min_size %d.  One warm-up per mode, then %d timed passes per mode, the modes alternating pass by "
             "pass; context profiling on (HIP events around every kernel launch); wall time around the call of the Python binding.  Median (min .. max) over the passes." %
             ("".join(" --%s %s" % (k, v) for k, v in (("templates", args.templates), ("passes", args.passes)) if v and (k, v) != ("passes", 3)), T, tbases / 1e9, len(rec),
              shape[6][0], threads, min_cov, min_size, args.passes), "",
             "The plan: %d effective ranges, %d segments over %.3f G positions, %d windows (one per %.1f segment positions)." %
             (len(p["eranges"]), len(p["segments"]), positions / 1e9, len(p["windows"]), positions / max(1, len(p["windows"]))), "",
             "| call | wall per pass (s) | `cns_table_finish` (ms) | `cns_plan_segments` (ms) | `cns_plan_count` (ms) | `cns_plan_emit` (ms) | scan + compact (ms) |", "|---|---|---|---|---|---|---|"]
    if parent:
        lines.append("| parent commit's library, `_ex`, TABLE (child process, same session) | %s | %.2f | | | | |" % (spread(parent["walls"]), float(np.median(parent["finish_ms"] or [0.0]))))
    for label, m in modes:
        lines.append("| %s | %s | %.2f | %.2f | %.2f | %.2f | %.2f |" % (label, spread(walls[m]), med(m, "cns_table_finish"), med(m, "cns_plan_segments"), med(m, "cns_plan_count"),
                                                                  med(m, "cns_plan_emit"), med(m, "cns_plan_scan") + med(m, "cns_plan_compact")))
    nsl = int(host[6]["slices"][0]) if host[6]["slices"] else 0
    lines += ["", "Plans of `TABLE | PLAN` and `PLAN` are equal byte for byte: %s." % same, "",
              "What the plan costs the host, from the call's own clock (`MECAT_CNS_TIMES=1`), seconds per pass, the batch in %d slices:" % nsl, "",
              "| call | waiting for the counts | putting the slices' pieces together |", "|---|---|---|"]
    for label, m in modes[1:]:
        lines.append("| %s | %s | %s |" % (label, spread(host[m]["wait"] or [0.0]), spread(host[m]["put"] or [0.0])))
    lines += ["", "The wait is the host blocked on the stream once per slice, until that slice's strings, tally, finish and plan kernels up to the window count have "
              "run (the windows' buffer is sized by their number); without the plan the host goes on to replay the next slice at once, so this is overlap that "
              "the plan modes give up, and it is part of their wall time above.  With more than one slice every segment and window record is copied once more "
              "on the host, from its slice's piece into the final buffer (%.2f GB of windows here): the second column." % (16.0 * len(p["windows"]) / 1e9), "",
              "All plan kernels together: **%.2f ms per pass** (TABLE | PLAN).  The expectation, stated and not enforced: about what `cns_table_finish` costs, %.0f ms per pass in "
              "`profiles/cns_table.md` (here: %.2f ms) — the plan reads 4 bytes per table position once (segments) and 1 + 5 bytes per segment position (count, emit) and writes "
              "16 bytes per window." % (plan_ms, FINISH_MS_EXPECTED, med(6, "cns_table_finish")), ""]
    if plan_ms > 3 * FINISH_MS_EXPECTED:
        worst = max(PLAN_KERNELS, key=lambda k: med(6, k))
        lines += ["That is more than three times the expectation.  Where the time goes: `%s` takes %.2f ms of it (%s)." %
                  (worst, med(6, worst), ", ".join("`%s` %.2f" % (k, med(6, k)) for k in PLAN_KERNELS)), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
