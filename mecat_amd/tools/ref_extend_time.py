#!/usr/bin/env python3
"""Times mecat2ref's extension stage on the device (mhip_ref_extend_run, mecat_amd/csrc/ref_extend.hip) and writes profiles/ref_extend.md:
    python -m mecat_amd.tools.ref_extend_time [--reads 20000] [--length 10000] [--err 0.15] [--genome 5000000] [--go-seconds S --go-bases B]
The workload is ref_seed_time's (libsynth): a genome of --genome bases as the reference, --reads reads of --length letters at --err from
both strands.  The round-1 candidate lists (-n 10) are made once by mhip_ref_seed_reads_dev and stay on the device; mhip_ref_extend_run_dev
extends them: one warm-up call, then five timed ones.  Kernel times are the HIP events per kernel name (mhip_ctx_kernel_stats), the median
of the five calls with their range; wall = the host clock around the call (it ends in a device synchronise).  --go-seconds / --go-bases
record, next to these numbers, the unmodified tool's own single-thread time in extend_candidate and the query bases it aligned, as the
fixture generator (tests/golden/make_golden_ref_ext.py) measured them on its machine."""
import argparse
import ctypes as C
import os
import statistics
import time

import numpy as np

from mecat_amd import hip as M
from mecat_amd import workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = ("ref_jobs", "ref_scan", "ref_extend", "ref_stitch", "ref_join")
DW_RATE = 21_520_149_150 / ((237.87 + 4.62) * 1e-3)          # profiles/dw_ring_linear.md: aligned_bases per step over dw_extend2 + dw_extend


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--err", type=float, default=0.15)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--seed", type=int, default=20262)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--go-seconds", type=float, default=None)
    ap.add_argument("--go-bases", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_extend.md"))
    a = ap.parse_args()
    lib = W.synth_lib()
    g = np.empty(a.genome, dtype=np.uint8)
    lib.synth_genome(g.ctypes.data, a.genome, a.seed)
    codes, lens = W.synth_reads(a.reads, a.length, a.err, a.genome, a.seed)
    ctx = M.Context(0)
    rpac, roffs, rnb = W.pack_volume(g, np.array([a.genome], dtype=np.int32))
    # the reference as ref_genome.cpp makes it: no pad base, so a position is an index (one record of A, C, G, T only)
    ref = M.Volume(ctx, rpac, np.array([[0, a.genome]], dtype=np.int32), a.genome, 0)
    idx = M.Index(ctx, ref)
    qpac, qoffs, qnb = W.pack_volume(codes, lens)
    reads = M.Volume(ctx, qpac, qoffs, qnb, 0)          # upper-case A, C, G, T only: no N plane needed
    n, maxc = a.reads, 10
    d_out, d_cnt = C.c_void_p(), C.c_void_p()
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"time_rx_out", n * maxc * M.REF_CAND_DTYPE.itemsize, C.byref(d_out)))
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"time_rx_cnt", n * 4, C.byref(d_cnt)))
    M.ref_seed_reads_dev(ctx, idx, ref, reads, 0, n, M.ref_seed_params(0, maxc=maxc, round=0), d_out, d_cnt)
    tot = M.ref_extend_run_dev(ctx, ref, reads, 0, n, maxc, d_out, d_cnt)          # warm-up: buffers allocated, code loaded
    ctx.set_profiling(True)
    per, wall = {k: [] for k in KERNELS}, []
    for _ in range(a.repeats):
        ctx.reset_stats()
        t0 = time.perf_counter()
        tot = M.ref_extend_run_dev(ctx, ref, reads, 0, n, maxc, d_out, d_cnt)
        wall.append((time.perf_counter() - t0) * 1e3)
        ks = ctx.kernel_stats()
        for k in KERNELS:
            per[k].append(ks.get(k, (0, 0.0))[1])
    ctx.set_profiling(False)
    st = M.ref_extend_stats()
    t0 = time.perf_counter()
    res, offs, words = M.ref_extend_fetch(ctx, n, maxc, tot)
    fetch_ms = (time.perf_counter() - t0) * 1e3
    flat = res.reshape(-1)
    jobs = int((flat["qs"] > 0).sum())
    ok = flat["ok"] == 1
    q_all = int((flat["qe"] - flat["qb"]).astype(np.int64).sum())
    q_ok = int((flat["qe"] - flat["qb"]).astype(np.int64)[ok].sum())
    med = {k: statistics.median(v) for k, v in per.items()}
    ext = med["ref_extend"]
    total = sum(med.values())
    with open(a.out, "w") as f:
        f.write("# mecat2ref extension stage on the device (ref_extend.hip): first measurement\n\n")
        f.write("Written by `python -m mecat_amd.tools.ref_extend_time`. Workload: %d synthetic reads of %d letters at %.0f %% error, both strands,\n"
                "against a synthetic reference of %d bases; the round-1 candidate lists (-n 10) of `mhip_ref_seed_reads_dev`, left on the device,\n"
                "through `mhip_ref_extend_run_dev`. One warm-up call, then %d timed calls; kernel ms = HIP events per kernel name\n"
                "(`mhip_ctx_kernel_stats`), median (min - max); wall ms = the whole call, which ends in a device synchronise.\n\n" % (
                    a.reads, a.length, a.err * 100, a.genome, a.repeats))
        f.write("| kernel | ms |\n|---|---|\n")
        for k in KERNELS:
            f.write("| `%s` | %.3f (%.3f - %.3f) |\n" % (k, med[k], min(per[k]), max(per[k])))
        f.write("| all kernels | %.3f |\n| `mhip_ref_extend_run_dev`, wall | %.2f (%.2f - %.2f) |\n| `mhip_ref_extend_fetch`, wall (once) | %.2f |\n\n" % (
            total, statistics.median(wall), min(wall), max(wall), fetch_ms))
        f.write("A call is %.0f ms of kernel time, which is short for a clock: hence the repeats, and their range beside every median.\n\n" % total)
        f.write("| jobs (occupied slots) | results of 1 000 columns or more | query bases aligned, all jobs | of the ok results | column words moved | slices | row scratch, bytes | column store, words |\n")
        f.write("|---|---|---|---|---|---|---|---|\n")
        f.write("| %d | %d | %d | %d | %d | %d | %d | %d |\n\n" % (jobs, int(ok.sum()), q_all, q_ok, tot, st["slices"], st["row_bytes"], st["store_words"]))
        f.write("Aligned query bases per second of `ref_extend` kernel time: **%.3g** over all jobs, %.3g counting the ok results only (the way the\n"
                "`aligned_bases` counter of the dw extension counts).\n\n" % (q_all / (ext * 1e-3), q_ok / (ext * 1e-3)))
        f.write("## Two yardsticks\n\n")
        f.write("* The counts-only dw extension (`dw_extend2` + `dw_extend`, `profiles/dw_ring_linear.md`): 21 520 149 150 aligned bases in 237.87 + 4.62 ms\n"
                "  = %.3g aligned bases per second, on mecat2pw's workload (read against read, ok results only). This stage runs at %.1f %% of that\n"
                "  rate by the same count. It does more per base: every d-row goes to global memory, the whole path is walked back and written out.\n" % (
                    DW_RATE, 100.0 * (q_ok / (ext * 1e-3)) / DW_RATE))
        if a.go_seconds is not None and a.go_bases is not None:
            f.write("* The unmodified tool's own `extend_candidate`, ONE CPU THREAD ON A DIFFERENT MACHINE, for scale only: %.3f s for the fixture's\n"
                    "  candidates (tests/golden/ref_ext.npz, %d query bases aligned) = %.3g bases per second.\n" % (a.go_seconds, a.go_bases, a.go_bases / a.go_seconds))
        f.write("\nNo threshold is set for this stage: these are its first measurements.\n\n")
        f.write("## What nobody has tuned\n\n"
                "* `ref_extend` is dw_extend's mapping with cns_extend's row log: no register-resident fast rows, no two units per wave, 16-base\n"
                "  snake steps, every row written to global memory and read back by one scalar walk per block.\n"
                "* 16 waves per CU is dw_extend's number, not a measured one (94 VGPRs and 5.6 KB of LDS per wave allow 20).\n"
                "* Units are taken in slot order; empty slots cost a cursor step each; long jobs are not started first.\n"
                "* `ref_join` reads the two directions' columns 2 bits at a time.\n"
                "* The column store is zero-filled per slice and the columns are set with atomic ORs.\n")
    print(open(a.out).read())
    idx.free(); ref.free(); reads.free(); ctx.close()


if __name__ == "__main__":
    main()
