#!/usr/bin/env python3
"""What the POA consensus of the listed windows costs in the accept stage: config 4's batch (every template of config 2's own overlaps,
as tools/cns_pieces_time.py builds it; its first 10 000 templates by default) through

    parent commit's library   mhip_cns_accept_templates_pieces  PLAN | PIECES   (--parent-tree DIR, a child process of this tool)
    this library              mhip_cns_accept_templates_poa     PLAN | PIECES   the call without the bit: must cost what the parent's costs
    this library              mhip_cns_accept_templates_poa     PLAN | POA      plan and consensus: no strings, tables or pieces cross the link

one warm-up per mode, then `--passes` timed passes per mode, the modes ALTERNATING pass by pass, with context profiling on so that the
cns_poa_* kernels appear in the kernel statistics (HIP events around every launch) and MECAT_CNS_TIMES=1, whose stderr lines give the
host waits and how many windows went to cns_poa_large.  Wall time is taken around the call of the Python binding, a device-wide wait on
either side.  The parent's passes are measured by a child process in the same session, started once this process has freed its volume
and closed its context, with the parent's own mecat_amd package (`make hip synth` in a checkout of the parent commit).

    python tools/cns_poa_time.py --reference-leg FILE     (CPU only, where the reference is built) the unmodified meap_cns_one_indel on
                                                          one thread over the windows of tests/golden/cns_poa.npz, through
                                                          tests/golden/cns_poa_ref_main.cpp -> windows/s as JSON in FILE
    python tools/cns_poa_time.py [--templates N] [--passes K] [--parent-tree DIR] [--ref-json FILE] [--out FILE]

Writes a small markdown report (default profiles/cns_poa.md).  Measures; asserts only that the plans of the modes are equal."""
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
POA_KERNELS = ("cns_poa_bound", "cns_poa_scan", "cns_poa_small", "cns_poa_list", "cns_poa_large", "cns_poa_widen", "cns_poa_gather")
PIECE_KERNELS = ("cns_pieces_tmplwin", "cns_pieces_mark", "cns_pieces_range", "cns_pieces_scan", "cns_pieces_cols", "cns_pieces_count", "cns_pieces_emit")


def spread(x):
    return "%.3f (%.3f .. %.3f)" % (float(np.median(x)), min(x), max(x)) if len(x) else "-"


def reference_leg(path, repeats=5):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cns_poa_cases as P
    cases, _ = P.load_fixture()
    nwin = sum(len(c["windows"]) for c in cases)
    with tempfile.TemporaryDirectory() as tmp:
        exe = P.build_ref_program(tmp)
        fin, fout = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "out.bin")
        P.write_cases(fin, cases)
        env = dict(os.environ, OMP_NUM_THREADS="1")
        subprocess.run([exe, fin, fout], check=True, env=env)
        dt = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            subprocess.run([exe, fin, fout], check=True, env=env)
            dt.append(time.perf_counter() - t0)
    res = dict(windows=nwin, seconds=dt, windows_per_s=nwin / float(np.median(dt)))
    json.dump(res, open(path, "w"))
    print(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--templates", type=int, default=10000, help="first N templates only (0: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cns_poa.md"))
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: its `_pieces` PLAN | PIECES passes, from a child process")
    ap.add_argument("--ref-json", default="", help="what --reference-leg wrote")
    ap.add_argument("--reference-leg", default="", help="run the reference leg (CPU) and write its result to this file")
    ap.add_argument("--pieces-only-json", action="store_true", help="(the child) mhip_cns_accept_templates_pieces, PLAN | PIECES passes only, one JSON line on stdout")
    ap.add_argument("--tree", default=ROOT, help="(the child) where mecat_amd is imported from")
    args = ap.parse_args()
    if args.reference_leg:
        return reference_leg(args.reference_leg)
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
    print("[cns_poa_time] %d templates, %d records, %.2f Gbase of templates, set up in %.1f s" % (T, len(rec), tbases / 1e9, time.time() - t0), file=sys.stderr, flush=True)
    mas, ratio = (params.min_align_size if ont else 2000), (0.4 if ont else 0.9)
    min_cov, min_size = (6, 2000) if ont else (4, 5000)          # mecat2cns' defaults
    PL, PC = 4, 8
    PO = 0 if args.pieces_only_json else M.CNS_WANT_POA

    def call(mode):
        r = rec.copy()
        ctx.sync()
        sys.stderr.flush()
        keep = os.dup(2)
        with tempfile.TemporaryFile() as tmp:       # the library's stderr lines of this call
            os.dup2(tmp.fileno(), 2)
            try:
                c0 = time.perf_counter()
                f = M.cns_accept_templates_pieces if args.pieces_only_json else M.cns_accept_templates_poa
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

    modes = [("`_pieces`, PLAN \\| PIECES", PL | PC)] if args.pieces_only_json else [("`_poa`, PLAN \\| PIECES", PL | PC), ("`_poa`, PLAN \\| POA", PL | PO)]
    ctx.set_profiling(True)
    walls = {m: [] for _, m in modes}
    kms = {m: {} for _, m in modes}
    plans, nacc = {}, 0
    host = {m: dict(wait=[], large=[], launches=[], slices=[]) for _, m in modes}      # from the library's stderr lines
    for _, m in modes:
        call(m)                                     # warm-up: scratch buffers, result buffers, page locking
    for _ in range(args.passes):
        for _, m in modes:                          # alternating: a drift of the host hits every mode alike
            ctx.reset_stats()
            dt, out, text = call(m)
            walls[m].append(dt)
            for key, pat in (("wait", r"waited for the counts ([0-9.]+)"), ("large", r"(\d+) windows in cns_poa_large"), ("launches", r"cns_poa_large \((\d+) launches"),
                             ("slices", r"jobs in (\d+) slices")):
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
    if args.pieces_only_json:
        print(json.dumps(dict(walls=walls[PL | PC], templates=T)))
        return
    p, q = plans[PL | PC], plans[PL | PO]
    same = all(p[k].tobytes() == q[k].tobytes() for k in ("segments", "seg_begin", "windows", "eranges", "erange_begin"))
    assert same, "the plans of PLAN | PIECES and PLAN | POA differ"
    nwin, npc, nb = len(q["windows"]), len(p["pieces"]), len(q["cns"])
    lens_w = np.diff(q["cns_begin"])

    parent = None
    if args.parent_tree:
        cmd = [sys.executable, os.path.abspath(__file__), "--pieces-only-json", "--tree", os.path.abspath(args.parent_tree), "--passes", str(args.passes),
               "--templates", str(args.templates)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=1500, check=True)
        parent = json.loads(r.stdout.decode().strip().splitlines()[-1])

    med = lambda m, k: float(np.median(kms[m].get(k, [0.0])))
    poa = PL | PO
    poa_ms = sum(med(poa, k) for k in POA_KERNELS)
    large = int(host[poa]["large"][0]) if host[poa]["large"] else 0
    small_ms, large_ms = med(poa, "cns_poa_small"), med(poa, "cns_poa_large")
    lines = ["# The POA consensus of the listed windows in the accept stage: what it costs", "",
             "`python tools/cns_poa_time.py` on one MI355X: the first %d templates of config 4's batch (%.2f Gbase of templates, %d candidate records, %d accepted alignments), "
             "%d host threads, min_cov %d / min_size %d.  One warm-up per mode, then %d timed passes per mode, the modes alternating pass by pass; context profiling on (HIP "
             "events around every kernel launch); wall time around the call of the Python binding.  Median (min .. max) over the passes." %
             (T, tbases / 1e9, len(rec), nacc, threads, min_cov, min_size, args.passes), "",
             "The plan: %d segments, %d windows, %d pieces (%.2f per window).  The consensus: **%d bytes** (%.2f per window; %.1f %% of the windows give more than 2 letters, "
             "what `meap_consensus_one_segment` appends from)." % (len(q["segments"]), nwin, npc, npc / max(1, nwin), nb, nb / max(1, nwin), 100.0 * float((lens_w > 2).mean()) if nwin else 0.0), "",
             "| call | wall per pass (s) | host waits: plan + pieces + POA (s) |", "|---|---|---|"]
    if parent:
        lines.append("| parent commit's library, `_pieces`, PLAN \\| PIECES (child process, same session) | %s | |" % spread(parent["walls"]))
    for label, m in modes:
        lines.append("| %s | %s | %s |" % (label, spread(walls[m]), spread(host[m]["wait"])))
    lines += ["", "Plans of the two modes are equal byte for byte: %s.  The batch ran in %d slices; every slice waits once more with `POA` (the three totals that size the output, "
              "the slots and the large windows' buffer)." % (same, int(host[poa]["slices"][0]) if host[poa]["slices"] else 0), ""]
    if parent:
        a, b = parent["walls"], walls[PL | PC]
        lines += ["Requirement — `_poa` without the bit costs what the parent's `_pieces` costs, within the spread of the passes: parent %s s, this library %s s; the medians differ "
                  "by %+.3f s, the passes of either spread over %.3f s and %.3f s." % (spread(a), spread(b), float(np.median(b) - np.median(a)), max(a) - min(a), max(b) - min(b)), ""]
    lines += ["POA kernels, ms per pass (PLAN | POA):", "", "| " + " | ".join("`%s`" % k for k in POA_KERNELS) + " | all |", "|" + "---|" * (len(POA_KERNELS) + 1),
              "| " + " | ".join("%.2f" % med(poa, k) for k in POA_KERNELS) + " | **%.2f** |" % poa_ms, "",
              "The piece kernels in the same passes: %.2f ms.  `cns_poa_scan` runs four times per slice, one block each, like `cns_pieces_scan`." % sum(med(poa, k) for k in PIECE_KERNELS), "",
              "`cns_poa_small` took %d of the %d windows (%.2f %%) in %.2f ms — %.1f M windows/s — and `cns_poa_large` the other %d in %.2f ms over %d launches: %.1f %% of the windows, "
              "%.1f %% of the two kernels' time." % (nwin - large, nwin, 100.0 * (nwin - large) / max(1, nwin), small_ms, (nwin - large) / max(small_ms, 1e-9) / 1e3, large, large_ms,
                                                   int(host[poa]["launches"][0]) if host[poa]["launches"] else 0, 100.0 * large / max(1, nwin), 100.0 * large_ms / max(small_ms + large_ms, 1e-9)), "",
              "The slot of `cns_poa_small` is %d words (%d KiB) per lane in global memory, two blocks of 256 lanes per CU resident: chosen before any measurement, as the size that "
              "holds a window of 20 positions with 10 pieces of 25 columns; the share of windows above is what it gives on this batch.  LDS was ruled out by size: 160 KB per CU "
              "hold ten such slots." % (M.cns_poa_small_words(), M.cns_poa_small_words() * 4 // 1024), ""]
    if args.ref_json and os.path.exists(args.ref_json):
        r = json.load(open(args.ref_json))
        lines += ["Reference leg — a CPU figure from ANOTHER machine (the build container), not comparable pass for pass: the unmodified `meap_cns_one_indel` on one thread over the "
                  "%d windows of `tests/golden/cns_poa.npz` (small synthetic windows, process start and file reading included), through `tests/golden/cns_poa_ref_main.cpp`: "
                  "%.0f windows/s (median of %d runs)." % (r["windows"], r["windows_per_s"], len(r["seconds"])), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
