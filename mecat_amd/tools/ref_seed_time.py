#!/usr/bin/env python3
"""Times mecat2ref's candidate stage on the device (mhip_ref_seed_reads, mecat_amd/csrc/ref_seed.hip) and writes profiles/ref_seed.md:
    python -m mecat_amd.tools.ref_seed_time [--reads 20000] [--length 10000] [--err 0.15] [--genome 5000000] [--ref-ms-per-read X]
The workload is synthetic (libsynth): a genome of --genome bases as the reference, --reads reads of --length letters at --err from both
strands.  Per round (0: 1 000-base segments, stride by length; 1: 2 000-base segments, stride 5) one warm-up call and three timed ones;
the kernel time is the sum of the events of `ref_seed` and `ref_seed_full` (the second launch for reads that outgrew their record pool),
the median of the three calls.  --ref-ms-per-read records, next to these numbers, a time measured elsewhere for the unmodified tool's
own stage (one CPU thread, both rounds, extension stubbed out by tests/golden/make_golden_ref_cand.py's recorder)."""
import argparse
import os
import statistics
import time

import numpy as np

from mecat_amd import hip as M
from mecat_amd import workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lookups(lens, rnd):
    """query k-mers of both strands: (len - 13) / BC + 1 each"""
    lens = lens.astype(np.int64)
    bc = np.full(len(lens), 5) if rnd else np.minimum(20, 5 + lens // 1000)
    return int(2 * np.where(lens >= 13, (lens - 13) // bc + 1, 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--err", type=float, default=0.15)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--seed", type=int, default=20262)
    ap.add_argument("--ref-ms-per-read", type=float, default=None)
    ap.add_argument("--ref-note", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_seed.md"))
    a = ap.parse_args()
    lib = W.synth_lib()
    g = np.empty(a.genome, dtype=np.uint8)
    lib.synth_genome(g.ctypes.data, a.genome, a.seed)
    codes, lens = W.synth_reads(a.reads, a.length, a.err, a.genome, a.seed)
    ctx = M.Context(0)
    rpac, roffs, rnb = W.pack_volume(g, np.array([a.genome], dtype=np.int32))
    ref = M.Volume(ctx, rpac, roffs, rnb, 0)
    t0 = time.perf_counter()
    idx = M.Index(ctx, ref)
    ctx.sync()
    index_ms = (time.perf_counter() - t0) * 1e3
    qpac, qoffs, qnb = W.pack_volume(codes, lens)
    reads = M.Volume(ctx, qpac, qoffs, qnb, 0)
    rows = []
    for rnd in (0, 1):
        p = M.ref_seed_params(0, round=rnd)
        M.ref_seed_reads(ctx, idx, ref, reads, 0, a.reads, p)          # warm-up: buffers allocated, code loaded
        ctx.set_profiling(True)
        kms, wall = [], []
        for _ in range(3):
            ctx.reset_stats()
            t0 = time.perf_counter()
            out, cnt = M.ref_seed_reads(ctx, idx, ref, reads, 0, a.reads, p)
            wall.append((time.perf_counter() - t0) * 1e3)
            ks = ctx.kernel_stats()
            kms.append(sum(v[1] for k, v in ks.items() if k in ("ref_seed", "ref_seed_full")))
        ctx.set_profiling(False)
        st = M.ref_seed_stats()
        km, wl = statistics.median(kms), statistics.median(wall)
        rows.append(dict(rnd=rnd, kernel_ms=km, wall_ms=wl, reads_per_s=a.reads / (km / 1e3), lookups=lookups(lens, rnd),
                         lookups_per_s=lookups(lens, rnd) / (km / 1e3), redone=st["redone"], waves=st["waves"], pool=st["pool"],
                         with_cands=int((cnt > 0).sum()), cands=int(cnt.sum()), spread=(min(kms), max(kms))))
    with open(a.out, "w") as f:
        f.write("# mecat2ref candidate stage on the device (ref_seed.hip)\n\n")
        f.write("Written by `python -m mecat_amd.tools.ref_seed_time`. Workload: %d synthetic reads of %d letters at %.0f %% error, both strands,\n"
                "against a synthetic reference of %d bases (index build, wall: %.1f ms). One warm-up call, then three timed calls per round;\n"
                "kernel ms = HIP events around `ref_seed` + `ref_seed_full`, median of three (min - max in brackets); wall ms = the whole\n"
                "`mhip_ref_seed_reads` call, lists copied to the host.\n\n" % (a.reads, a.length, a.err * 100, a.genome, index_ms))
        f.write("| round | kernel ms | wall ms | reads / s | k-mer look-ups | look-ups / s | reads redone with full pools | waves | pool records | reads with candidates | candidates |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %d | %.2f (%.2f - %.2f) | %.2f | %.0f | %d | %.3g | %d (%.2f %%) | %d | %d | %d | %d |\n" % (
                r["rnd"], r["kernel_ms"], r["spread"][0], r["spread"][1], r["wall_ms"], r["reads_per_s"], r["lookups"], r["lookups_per_s"], r["redone"],
                100.0 * r["redone"] / a.reads, r["waves"], r["pool"], r["with_cands"], r["cands"]))
        f.write("\nNo threshold is set for this stage: these are its first measurements.\n")
        if a.ref_ms_per_read is not None:
            both = sum(r["kernel_ms"] for r in rows) / a.reads
            f.write("\nThe unmodified tool's own stage, for scale only — A DIFFERENT MACHINE AND ONE CPU THREAD: %.3f ms per read for both rounds\n"
                    "(its `The Mapping Time` with the extension stubbed out by the fixture generator's recorder%s). The device's kernel time\n"
                    "for both rounds is %.4f ms per read.\n" % (a.ref_ms_per_read, a.ref_note and "; " + a.ref_note, both))
    print(open(a.out).read())
    idx.free(); ref.free(); reads.free(); ctx.close()


if __name__ == "__main__":
    main()
