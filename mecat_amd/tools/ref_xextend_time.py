#!/usr/bin/env python3
"""Times mecat2ref's extension stage in nanopore mode on the device (mhip_ref_xextend_run, mecat_amd/csrc/ref_xextend.hip) and writes
profiles/ref_xextend.md:
    python -m mecat_amd.tools.ref_xextend_time [--reads 20000] [--length 10000] [--err 0.15] [--genome 5000000] [--go-seconds S --go-bases B]
The workload is ref_extend_time's (libsynth): a genome of --genome bases as the reference, --reads reads of --length letters at --err from
both strands, the round-1 candidate lists (-n 10) made once by mhip_ref_seed_reads_dev and left on the device.  The same lists go through
mhip_ref_xextend_run_dev (the X-drop aligner) and, beside it, through mhip_ref_extend_run_dev (the O(ND) aligner): one warm-up call each,
then five timed ones.  Kernel times are the HIP events per kernel name (mhip_ctx_kernel_stats), the median of the five calls with their
range; wall = the host clock around the call (it ends in a device synchronise).  --go-seconds / --go-bases record, next to these
numbers, the unmodified tool's own single-thread time in extend_candidate with an XdropAligner and the query bases it aligned, as the
fixture generator (tests/golden/make_golden_ref_xext.py) measured them on its machine."""
import argparse
import ctypes as C
import os
import statistics
import time

import numpy as np

from mecat_amd import hip as M
from mecat_amd import workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = {"x": ("ref_jobs", "ref_scan", "ref_xextend", "ref_stitch", "ref_join"), "d": ("ref_jobs", "ref_scan", "ref_extend", "ref_stitch", "ref_join")}


def timed(ctx, run, kernels, repeats):
    tot = run()          # warm-up: buffers allocated, code loaded
    ctx.set_profiling(True)
    per, wall = {k: [] for k in kernels}, []
    for _ in range(repeats):
        ctx.reset_stats()
        t0 = time.perf_counter()
        tot = run()
        wall.append((time.perf_counter() - t0) * 1e3)
        ks = ctx.kernel_stats()
        for k in kernels:
            per[k].append(ks.get(k, (0, 0.0))[1])
    ctx.set_profiling(False)
    return tot, per, wall


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_xextend.md"))
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
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"time_rxx_out", n * maxc * M.REF_CAND_DTYPE.itemsize, C.byref(d_out)))
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"time_rxx_cnt", n * 4, C.byref(d_cnt)))
    M.ref_seed_reads_dev(ctx, idx, ref, reads, 0, n, M.ref_seed_params(0, maxc=maxc, round=0), d_out, d_cnt)
    dtot, dper, dwall = timed(ctx, lambda: M.ref_extend_run_dev(ctx, ref, reads, 0, n, maxc, d_out, d_cnt), KERNELS["d"], a.repeats)
    dres, _, _ = M.ref_extend_fetch(ctx, n, maxc, dtot)
    xtot, xper, xwall = timed(ctx, lambda: M.ref_xextend_run_dev(ctx, ref, reads, 0, n, maxc, d_out, d_cnt), KERNELS["x"], a.repeats)
    st = M.ref_xextend_stats()
    t0 = time.perf_counter()
    res, offs, words = M.ref_extend_fetch(ctx, n, maxc, xtot)
    fetch_ms = (time.perf_counter() - t0) * 1e3
    flat, dflat = res.reshape(-1), dres.reshape(-1)
    jobs = int((flat["qs"] > 0).sum())
    ok = flat["ok"] == 1
    q_all = int((flat["qe"] - flat["qb"]).astype(np.int64).sum())
    dq_all = int((dflat["qe"] - dflat["qb"]).astype(np.int64).sum())
    med = {k: statistics.median(v) for k, v in xper.items()}
    dmed = {k: statistics.median(v) for k, v in dper.items()}
    with open(a.out, "w") as f:
        f.write("# mecat2ref extension stage in nanopore mode on the device (ref_xextend.hip): first measurement\n\n")
        f.write("Written by `python -m mecat_amd.tools.ref_xextend_time`. Workload: %d synthetic reads of %d letters at %.0f %% error, both strands,\n"
                "against a synthetic reference of %d bases; the round-1 candidate lists (-n 10) of `mhip_ref_seed_reads_dev`, left on the device,\n"
                "through `mhip_ref_xextend_run_dev` and, beside it, the same lists through `mhip_ref_extend_run_dev` (the O(ND) aligner). One\n"
                "warm-up call each, then %d timed calls; kernel ms = HIP events per kernel name (`mhip_ctx_kernel_stats`), median (min - max);\n"
                "wall ms = the whole call, which ends in a device synchronise.\n\n" % (a.reads, a.length, a.err * 100, a.genome, a.repeats))
        f.write("| kernel | X-drop, ms | O(ND), ms |\n|---|---|---|\n")
        for kx, kd in zip(KERNELS["x"], KERNELS["d"]):
            f.write("| `%s` / `%s` | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) |\n" % (kx, kd, med[kx], min(xper[kx]), max(xper[kx]), dmed[kd], min(dper[kd]), max(dper[kd])))
        f.write("| all kernels | %.3f | %.3f |\n| the call, wall | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) |\n| `mhip_ref_extend_fetch`, wall (once) | %.2f | |\n\n" % (
            sum(med.values()), sum(dmed.values()), statistics.median(xwall), min(xwall), max(xwall), statistics.median(dwall), min(dwall), max(dwall), fetch_ms))
        f.write("| jobs (occupied slots) | ok results (query span of 1 000 or more) | query bases aligned, all jobs | the same, O(ND) | column words moved | slices | blocks redone with the wide block | column store, words |\n")
        f.write("|---|---|---|---|---|---|---|---|\n")
        f.write("| %d | %d | %d | %d | %d | %d | %d | %d |\n\n" % (jobs, int(ok.sum()), q_all, dq_all, xtot, st["slices"], st["redone"], st["store_words"]))
        f.write("Aligned query bases per second of `ref_xextend` kernel time: **%.3g**; of `ref_extend` kernel time on the same lists: %.3g.\n\n" % (
            q_all / (med["ref_xextend"] * 1e-3), dq_all / (dmed["ref_extend"] * 1e-3)))
        if a.go_seconds is not None and a.go_bases is not None:
            f.write("The unmodified tool's own `extend_candidate` with an `XdropAligner`, ONE CPU THREAD ON A DIFFERENT MACHINE, for scale only: %.3f s for\n"
                    "the fixture's candidates (tests/golden/ref_xext.npz, %d query bases aligned) = %.3g bases per second.\n\n" % (
                        a.go_seconds, a.go_bases, a.go_bases / a.go_seconds))
        f.write("No threshold is set for this stage: these are its first measurements, and parity with the tool is its gate.\n\n")
        f.write("## What nobody has tuned\n\n"
                "* The blocks are `xd_extend_w`'s; what is new per block is the column sink (one LDS OR per gap column from lane 0), the append\n"
                "  (16 two-bit reads per output word, atomic ORs into the store) and the re-zeroing of the 92-word buffer.\n"
                "* 8 waves per CU, because every wave owns 583 KB of wide state in global memory; `xd_extend_w` runs 24.\n"
                "* Units are taken in slot order, not longest first; empty slots cost a cursor step each.\n"
                "* A false candidate's extension drifts through unrelated sequence, where the window outgrows the ring: those blocks run twice\n"
                "  (ring, then wide on global state).  On mecat2ref's lists that is far from rare.\n")
    print(open(a.out).read())
    idx.free(); ref.free(); reads.free(); ctx.close()


if __name__ == "__main__":
    main()
