#!/usr/bin/env python3
"""What the POA windows' pieces cost in the accept stage: config 4's batch (every template of config 2's own overlaps, as
tools/cns_plan_time.py builds it; by default its first 10 000 templates, the subset bench.py's cns_accept times — the whole batch is
about 1.5 G pieces of 16 bytes on the host) through

    mhip_cns_accept_templates_pieces  PLAN            the plan alone, as mhip_cns_accept_templates_plan gives it
                                      PLAN | PIECES   plan and pieces: neither strings nor tables cross the PCIe link

one warm-up each, then `--passes` timed passes per mode, the modes ALTERNATING pass by pass, with context profiling on so that the
cns_pieces_* kernels appear in the kernel statistics (HIP events around every launch) and MECAT_CNS_TIMES=1, whose stderr lines say how
long the host waited (the plan's wait for the window count and the pieces' wait for their bound, once per slice each) and how long the
hand-over took (the slices' records put together).  --parent-tree DIR: a checkout of the parent commit with its library built
(`make hip synth`); its `_plan` PLAN passes are measured by a child process of this tool in the same session, started once this
process has freed its volume and closed its context, with the parent's own mecat_amd package.  Wall time is taken around the call of
the Python binding, a device-wide wait on either side.  Writes a small markdown report (default profiles/cns_pieces.md).  Measures;
asserts only that the plans of the two modes are equal.

    python tools/cns_pieces_time.py [--templates N] [--passes K] [--parent-tree DIR] [--out FILE]
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
TALLY_MS_EXPECTED = 99.0        # cns_table_tally per pass over the whole batch in profiles/cns_table.md: the boundary walk reads the same columns
PIECE_KERNELS = ("cns_pieces_tmplwin", "cns_pieces_mark", "cns_pieces_range", "cns_pieces_scan", "cns_pieces_cols", "cns_pieces_count", "cns_pieces_emit")


def spread(x):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(x)), min(x), max(x)) if len(x) else "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--templates", type=int, default=10000, help="first N templates only (0: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cns_pieces.md"))
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: its PLAN passes, from a child process")
    ap.add_argument("--plan-only-json", action="store_true", help="(the child) mhip_cns_accept_templates_plan, PLAN passes only, one JSON line on stdout")
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
    whole = T == len(ids)
    rec = np.ascontiguousarray(rec[: tb[T]])
    tb = tb[: T + 1]
    tbases = int(lens[ids[:T]].astype(np.int64).sum())
    threads = int(os.environ.get("MECAT_BENCH_THREADS", min(64, os.cpu_count() or 1)))
    print("[cns_pieces_time] %d templates, %d records, %.2f Gbase of templates, set up in %.1f s" % (T, len(rec), tbases / 1e9, time.time() - t0), file=sys.stderr, flush=True)
    mas, ratio = (params.min_align_size if ont else 2000), (0.4 if ont else 0.9)
    min_cov, min_size = (6, 2000) if ont else (4, 5000)          # mecat2cns' defaults
    PL = 4
    PC = 0 if args.plan_only_json else M.CNS_WANT_PIECES

    def call(mode):
        r = rec.copy()
        ctx.sync()
        sys.stderr.flush()
        keep = os.dup(2)
        with tempfile.TemporaryFile() as tmp:       # the library's stderr lines of this call
            os.dup2(tmp.fileno(), 2)
            try:
                c0 = time.perf_counter()
                f = M.cns_accept_templates_plan if args.plan_only_json else M.cns_accept_templates_pieces
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

    modes = [("`_plan`, PLAN", PL)] if args.plan_only_json else [("`_pieces`, PLAN", PL), ("`_pieces`, PLAN \\| PIECES", PL | PC)]
    ctx.set_profiling(True)
    walls = {m: [] for _, m in modes}
    kms = {m: {} for _, m in modes}
    plans, nacc = {}, 0
    host = {m: dict(wait=[], put=[], last=[], slices=[]) for _, m in modes}      # from the library's stderr lines
    for _, m in modes:
        call(m)                                     # warm-up: scratch buffers, result buffers, page locking
    for _ in range(args.passes):
        for _, m in modes:                          # alternating: a drift of the host hits every mode alike
            ctx.reset_stats()
            dt, out, text = call(m)
            walls[m].append(dt)
            for key, pat in (("wait", r"waited for the counts ([0-9.]+)"), ("put", r"put together ([0-9.]+)"), ("last", r"last copies ([0-9.]+)"), ("slices", r"jobs in (\d+) slices")):
                f = re.search(pat, text)
                if f:
                    host[m][key].append(float(f.group(1)))
            for k, (launches, ms) in ctx.kernel_stats().items():
                kms[m].setdefault(k, []).append(ms)
            plans[m] = out[6]
            nacc = len(out[0])
            del out
    ctx.set_profiling(False)
    vol.free()
    ctx.close()
    if args.plan_only_json:
        print(json.dumps(dict(walls=walls[PL], templates=T)))
        return
    p, q = plans[PL], plans[PL | PC]
    same = all(p[k].tobytes() == q[k].tobytes() for k in p)
    assert same, "the plans of PLAN and PLAN | PIECES differ"
    npc, nwin = len(q["pieces"]), len(q["windows"])

    parent = None
    if args.parent_tree:
        cmd = [sys.executable, os.path.abspath(__file__), "--plan-only-json", "--tree", os.path.abspath(args.parent_tree), "--passes", str(args.passes),
               "--templates", str(args.templates)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=1500, check=True)
        parent = json.loads(r.stdout.decode().strip().splitlines()[-1])

    med = lambda m, k: float(np.median(kms[m].get(k, [0.0])))
    both = PL | PC
    piece_ms = sum(med(both, k) for k in PIECE_KERNELS)
    share = tbases / 1.58e9 if not whole else 1.0      # (profiles/cns_plan.md: the whole batch is 1.58 G table positions)
    lines = ["# The POA windows' pieces in the accept stage: what they cost", "",
             "`python tools/cns_pieces_time.py%s` on one MI355X: %s (%d templates, %.2f Gbase of templates, %d candidate records, %d accepted alignments), %d host threads, "
             "min_cov %d / min_size %d.  One warm-up per mode, then %d timed passes per mode, the modes alternating pass by pass; context profiling on (HIP events around every "
             "kernel launch); wall time around the call of the Python binding.  Median (min .. max) over the passes." %
             ("".join(" --%s %s" % (k, v) for k, v in (("templates", args.templates), ("passes", args.passes)) if (k, v) not in (("templates", 10000), ("passes", 5))),
              "config 4's whole batch" if whole else "the first %d templates of config 4's batch — the subset bench.py's cns_accept times; the whole batch's pieces, about 1.5 G "
              "records of 16 bytes, are more than a host buffer should be asked for here" % T, T, tbases / 1e9, len(rec), nacc, threads, min_cov, min_size, args.passes), "",
             "The plan: %d segments, %d windows.  The pieces: **%d** (%.2f per window, %.2f GB of records)." % (len(q["segments"]), nwin, npc, npc / max(1, nwin), 16.0 * npc / 1e9), "",
             "| call | wall per pass (s) | host waits, plan + pieces (s) | hand-over: slices put together (s) | last copies, hand-over included (s) |", "|---|---|---|---|---|"]
    if parent:
        lines.append("| parent commit's library, `_plan`, PLAN (child process, same session) | %s | | | |" % spread(parent["walls"]))
    for label, m in modes:
        lines.append("| %s | %s | %s | %s | %s |" % (label, spread(walls[m]), spread(host[m]["wait"]), spread(host[m]["put"]), spread(host[m]["last"])))
    lines += ["", "Plans of `PLAN` and `PLAN | PIECES` are equal byte for byte: %s.  The batch ran in %d slices." % (same, int(host[both]["slices"][0]) if host[both]["slices"] else 0), "",
              "Piece kernels, ms per pass (PLAN | PIECES):", "", "| " + " | ".join("`%s`" % k for k in PIECE_KERNELS) + " | all |", "|" + "---|" * (len(PIECE_KERNELS) + 1),
              "| " + " | ".join("%.2f" % med(both, k) for k in PIECE_KERNELS) + " | **%.2f** |" % piece_ms, "",
              "The added host wait is the second column's difference: once per slice the host blocks until the slice's alignments have found their window ranges (the bound on "
              "the pieces sizes the boundary-column and piece buffers); the number of pieces itself is not waited for — every slice copies the slots its bound allows and the count "
              "is read at the hand-over.  With more than one slice every piece record is copied once more on the host, into the final buffer: the third column's difference.", "",
              "The expectation, stated and not enforced: `cns_pieces_cols` walks the columns `cns_table_tally` walks, %.0f ms per pass over the whole batch in `profiles/cns_table.md`, "
              "so about %.0f ms for this share of it (%.2f of the template bases); measured %.2f ms (`cns_table_tally` in the same passes: %.2f ms).  The window pass "
              "(`cns_pieces_count` + `cns_pieces_emit`) reads 8 bytes per overlapping pair twice plus 24 bytes of alignment record, and writes 16 bytes per piece: %.2f ms." %
              (TALLY_MS_EXPECTED, TALLY_MS_EXPECTED * share, share, med(both, "cns_pieces_cols"), med(both, "cns_table_tally"), med(both, "cns_pieces_count") + med(both, "cns_pieces_emit")), ""]
    worst = max(PIECE_KERNELS, key=lambda k: med(both, k))
    if worst == "cns_pieces_scan":
        lines += ["`cns_pieces_scan` is one block of 1 024 lanes over every alignment's and every window's count (%d windows here): %.2f of the %.2f ms, the largest share, and "
                  "the first thing to spread over the chip." % (nwin, med(both, worst), piece_ms), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
