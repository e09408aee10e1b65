#!/usr/bin/env python3
"""Times mecat2ref's rescue stage on the device (mhip_ref_rescue_run_dev, mecat_amd/csrc/ref_rescue.hip) and writes profiles/ref_rescue.md:
    python -m mecat_amd.tools.ref_rescue_time [--reads 20000] [--length 10000] [--err 0.15] [--genome 5000000] [--deleted 0.2]
                                              [--parent-lib PATH] [--resources FILE]
The workload is ref_seed_time's (libsynth): a genome of --genome bases as the reference, --reads reads of --length letters at --err from
both strands; a share --deleted of the reads loses 3 000 letters from its middle (a 3 kb deletion against the reference).  Round-1 lists
(-n 10) are made by mhip_ref_seed_reads_dev and extended by mhip_ref_extend_run_dev; mhip_ref_rescue_run_dev then works on the results
that stay on the device: one warm-up call, three timed ones, HIP events per kernel name, medians with their range.
ref_seed itself is measured again the way ref_seed_time does (one warm-up, three calls per round, on the same reads without the
deletions), in a child process per library: this build and, with --parent-lib, a build that differs only in ref_seed.hip being the
parent commit's.  --resources names a text file with the compiler's resource remarks of both, copied into the report."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

from mecat_amd import hip as M
from mecat_amd import workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = ("ref_rescue_prep", "ref_rescue_find", "ref_rescue_find_full", "ref_jobs", "ref_scan", "ref_extend", "ref_stitch", "ref_join", "ref_rescue_finish")


def workload(a, deleted):
    lib = W.synth_lib()
    g = np.empty(a.genome, dtype=np.uint8)
    lib.synth_genome(g.ctypes.data, a.genome, a.seed)
    codes, lens = W.synth_reads(a.reads, a.length, a.err, a.genome, a.seed)
    ncut = 0
    if deleted > 0:
        starts = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
        cut = np.random.default_rng(a.seed).random(len(lens)) < deleted
        parts, new = [], lens.copy()
        for i in range(len(lens)):
            r = codes[starts[i]: starts[i + 1]]
            if cut[i] and len(r) >= 9000:
                m = len(r) // 2
                r = np.concatenate([r[: m - 1500], r[m + 1500:]])
                ncut += 1
            new[i] = len(r)
            parts.append(r)
        codes, lens = np.concatenate(parts), new
    return g, codes, lens, ncut


def upload(a, g, codes, lens):
    ctx = M.Context(0)
    rpac, _, _ = W.pack_volume(g, np.array([a.genome], dtype=np.int32))
    # the reference as ref_genome.cpp makes it: no pad base, so a position is an index (one record of A, C, G, T only)
    ref = M.Volume(ctx, rpac, np.array([[0, a.genome]], dtype=np.int32), a.genome, 0)
    idx = M.Index(ctx, ref)
    qpac, qoffs, qnb = W.pack_volume(codes, lens)
    reads = M.Volume(ctx, qpac, qoffs, qnb, 0)          # upper-case A, C, G, T only: no N plane needed
    return ctx, ref, idx, reads


def seed_only(a):
    """ref_seed_time's measurement -> one JSON line {round: [kernel ms of the three calls]}"""
    g, codes, lens, _ = workload(a, 0.0)
    ctx, ref, idx, reads = upload(a, g, codes, lens)
    out = {}
    for rnd in (0, 1):
        p = M.ref_seed_params(0, round=rnd)
        M.ref_seed_reads(ctx, idx, ref, reads, 0, a.reads, p)
        ctx.set_profiling(True)
        kms = []
        for _ in range(3):
            ctx.reset_stats()
            M.ref_seed_reads(ctx, idx, ref, reads, 0, a.reads, p)
            ks = ctx.kernel_stats()
            kms.append(sum(v[1] for k, v in ks.items() if k in ("ref_seed", "ref_seed_full")))
        ctx.set_profiling(False)
        out[str(rnd)] = kms
    print("SEED_ONLY " + json.dumps(out))
    idx.free(); ref.free(); reads.free(); ctx.close()


def seed_child(a, libpath):
    env = dict(os.environ)
    if libpath:
        env["MECAT_HIP_LIB"] = libpath
    r = subprocess.run([sys.executable, "-m", "mecat_amd.tools.ref_rescue_time", "--seed-only", "--reads", str(a.reads), "--length", str(a.length), "--err", str(a.err),
                        "--genome", str(a.genome), "--seed", str(a.seed)], env=env, capture_output=True, text=True, cwd=ROOT, timeout=400)
    if r.returncode != 0:
        raise RuntimeError("ref_seed measurement failed: " + r.stderr[-2000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("SEED_ONLY ")][-1]
    return {int(k): v for k, v in json.loads(line[len("SEED_ONLY "):]).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--err", type=float, default=0.15)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--seed", type=int, default=20262)
    ap.add_argument("--deleted", type=float, default=0.2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--seed-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_rescue.md"))
    a = ap.parse_args()
    if a.seed_only:
        return seed_only(a)
    # ref_seed before / after, each in a process of its own (before this process opens the device)
    seed_parent = seed_child(a, a.parent_lib) if a.parent_lib else None
    seed_this = seed_child(a, None)
    g, codes, lens, ncut = workload(a, a.deleted)
    ctx, ref, idx, reads = upload(a, g, codes, lens)
    n, maxc = a.reads, 10
    d_out, d_cnt = C.c_void_p(), C.c_void_p()
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"time_rr_out", n * maxc * M.REF_CAND_DTYPE.itemsize, C.byref(d_out)))
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"time_rr_cnt", n * 4, C.byref(d_cnt)))
    M.ref_seed_reads_dev(ctx, idx, ref, reads, 0, n, M.ref_seed_params(0, maxc=maxc, round=0), d_out, d_cnt)
    M.ref_extend_run_dev(ctx, ref, reads, 0, n, maxc, d_out, d_cnt)
    p = M.ref_rescue_params(0, maxc=maxc, round=0, num_output=10)
    tot = M.ref_rescue_run_dev(ctx, idx, ref, reads, 0, n, p, None)          # warm-up: buffers allocated, code loaded
    ctx.set_profiling(True)
    per, wall = {k: [] for k in KERNELS}, []
    for _ in range(3):
        ctx.reset_stats()
        t0 = time.perf_counter()
        tot = M.ref_rescue_run_dev(ctx, idx, ref, reads, 0, n, p, None)
        wall.append((time.perf_counter() - t0) * 1e3)
        ks = ctx.kernel_stats()
        for k in KERNELS:
            per[k].append(ks.get(k, (0, 0.0))[1])
    ctx.set_profiling(False)
    st = M.ref_rescue_stats()
    out = M.ref_rescue_fetch(ctx, n, 10, tot)
    ok = int(out["res"]["ok"].sum())
    attached = int(((out["out_slots"] >= maxc) & (out["out_slots"] >= 0)).sum())
    with open(a.out, "w") as f:
        f.write("# mecat2ref rescue stage on the device (ref_rescue.hip): first measurement\n\n")
        f.write("Written by `python -m mecat_amd.tools.ref_rescue_time`. Workload: %d synthetic reads of %d letters at %.0f %% error, both strands,\n"
                "against a synthetic reference of %d bases; %d reads (%.1f %%) lost 3 000 letters from their middle. Round-1 lists (-n 10) seeded\n"
                "and extended on the device; `mhip_ref_rescue_run_dev` on the resident results: one warm-up call, three timed ones; kernel ms =\n"
                "HIP events per kernel name, median (min - max); whole call = the host clock around it (it ends in a device synchronise).\n\n"
                % (n, a.length, a.err * 100, a.genome, ncut, 100.0 * ncut / n))
        f.write("Reads that went on past the full-alignment test: %d of %d (%.1f %%); rescue candidates: %d (%d gave an ok result, %d records of\n"
                "rescue results are printed, i.e. attached or kept by the full-alignment cut); reads redone with full record pools: %d.\n\n"
                % (st["went_on"], n, 100.0 * st["went_on"] / n, st["candidates"], ok, attached, st["redone"]))
        f.write("| kernel | ms |\n|---|---|\n")
        for k in KERNELS:
            f.write("| %s | %.3f (%.3f - %.3f) |\n" % (k, statistics.median(per[k]), min(per[k]), max(per[k])))
        f.write("| all kernels | %.3f |\n" % sum(statistics.median(per[k]) for k in KERNELS))
        f.write("| whole call (wall) | %.3f (%.3f - %.3f) |\n" % (statistics.median(wall), min(wall), max(wall)))
        f.write("\nNo threshold is set for this stage: these are its first measurements. `ref_rescue_find` runs stage 1's seeding loop again for\n"
                "the strands that own one of a read's first three entries, for the reads that went on only.\n")
        f.write("\n## ref_seed before and after its seeding loop moved to ref_seed_dev.h\n\n")
        f.write("Measured as `ref_seed_time` measures it (the same reads without the deletions, one warm-up and three calls per round, kernel ms of\n"
                "`ref_seed` + `ref_seed_full`), each library in a process of its own in this session. \"Parent\" is a library that differs from this\n"
                "build only in `ref_seed.hip` being the parent commit's file.\n\n")
        f.write("| round | parent: median (min - max) | this build: median (min - max) | this median inside the parent's spread |\n|---|---|---|---|\n")
        for rnd in (0, 1):
            t = seed_this[rnd]
            if seed_parent:
                q = seed_parent[rnd]
                inside = min(q) <= statistics.median(t) <= max(q)
                f.write("| %d | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %s |\n" % (rnd, statistics.median(q), min(q), max(q), statistics.median(t), min(t), max(t),
                                                                                 "yes" if inside else "no: %.2f %% %s" % (abs(statistics.median(t) / statistics.median(q) - 1) * 100,
                                                                                                           "faster" if statistics.median(t) < statistics.median(q) else "slower")))
            else:
                f.write("| %d | not measured | %.3f (%.3f - %.3f) | - |\n" % (rnd, statistics.median(t), min(t), max(t)))
        if a.resources and os.path.exists(a.resources):
            f.write("\nThe compiler's resource remarks for `ref_seed` (gfx950, -O3 -ffp-contract=off):\n\n```\n%s\n```\n" % open(a.resources).read().strip())
    print(open(a.out).read())
    idx.free(); ref.free(); reads.free(); ctx.close()


if __name__ == "__main__":
    main()
