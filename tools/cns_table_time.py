#!/usr/bin/env python3
"""What the consensus table costs in the accept stage: config 4's batch (bench_config4.py: every template of config 2's own overlaps)
through

    mhip_cns_accept_templates                      the entry point as it was (strings only)
    mhip_cns_accept_templates_ex  STRINGS          the same through the new entry point
                                  STRINGS | TABLE  strings and tables
                                  TABLE            tables only: the strings stay on the device

one warm-up and two timed passes each, with context profiling on, so that cns_table_tally / cns_table_finish appear in the kernel
statistics.  Writes a small markdown report (default profiles/cns_table.md).  Measures; asserts only that the tables of the last two
modes are equal.  Reads nothing but this repository's own generator.

    python tools/cns_table_time.py [--templates N] [--out FILE]
"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ATOMIC_RATE_GUIDE = 1.3e12      # chip-wide global atomic adds, bytes added per second (measured for float adds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--templates", type=int, default=0, help="first N templates only (0: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cns_table.md"))
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as in the tests)
    from mecat_amd import hip as M, workload as W

    os.environ["MECAT_CNS_TIMES"] = "1"          # the call's own breakdown ("last copies") on stderr
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
    print("[cns_table_time] %d templates, %d records, %.2f Gbase of templates, set up in %.1f s" % (T, len(rec), tbases / 1e9, time.time() - t0), file=sys.stderr, flush=True)
    mas, ratio = (params.min_align_size if ont else 2000), (0.4 if ont else 0.9)

    def call(mode):
        r = rec.copy()
        ctx.sync()
        c0 = time.perf_counter()
        if mode is None:
            out = M.cns_accept_templates(ctx, vol, None, r, tb, ont, mas, ratio, threads=threads) + (np.zeros(0, M.TABLE_DTYPE), np.zeros(0, np.uint8), np.zeros(0, np.int64))
        else:
            out = M.cns_accept_templates_ex(ctx, vol, r, tb, ont, mas, ratio, mode, threads=threads)
        ctx.sync()
        return time.perf_counter() - c0, out

    ctx.set_profiling(True)
    modes = [("mhip_cns_accept_templates (as before)", None), ("_ex, STRINGS", M.CNS_WANT_STRINGS), ("_ex, STRINGS | TABLE", M.CNS_WANT_STRINGS | M.CNS_WANT_TABLE),
             ("_ex, TABLE", M.CNS_WANT_TABLE)]
    rows, keep = [], {}
    for label, mode in modes:
        print("[cns_table_time] --- %s" % label, file=sys.stderr, flush=True)
        call(mode)                                  # warm-up: scratch buffers, result buffers, page locking
        ctx.reset_stats()
        walls, out = [], None
        for _ in range(args.passes):
            out = None                              # (the previous pass's buffers go back before the next call asks for its own)
            dt, out = call(mode)
            walls.append(dt)
        ks = ctx.kernel_stats()
        acc, strs, nj, table, ident, begin = out
        adds = 0
        if len(table):
            h = hashlib.sha256()
            for o in range(0, len(table), 1 << 26):          # in pieces: the table of the whole batch is gigabytes
                piece = table[o: o + (1 << 26)]
                adds += int(piece.view(np.uint8).reshape(-1, 4)[:, 1:].sum(dtype=np.int64))
                h.update(piece)
            h.update(ident)
            keep[label] = h.hexdigest()
        rows.append(dict(label=label, walls=walls, accepted=len(acc), string_bytes=len(strs), columns=int(acc["aln_size"].astype(np.int64).sum()), words=len(table), adds=adds,
                         tally_ms=ks.get("cns_table_tally", (0, 0.0))[1] / args.passes, finish_ms=ks.get("cns_table_finish", (0, 0.0))[1] / args.passes,
                         strings_ms=(ks.get("cns_strings_build", (0, 0.0))[1] + ks.get("cns_push_gaps", (0, 0.0))[1]) / args.passes))
        del out, acc, strs, table, ident
    ctx.set_profiling(False)
    same = keep["_ex, STRINGS | TABLE"] == keep["_ex, TABLE"]
    assert same, "the tables of STRINGS | TABLE and TABLE differ"

    base = min(rows[0]["walls"])
    lines = ["# The consensus table in the accept stage: what it costs", "",
             "`python tools/cns_table_time.py%s` on one MI355X: config 4's batch (%d templates of config 2's overlaps, %.2f Gbase of templates, %d candidate records, "
             "%d accepted alignments, %.2f G columns), %d host threads; one warm-up and %d timed passes per mode, context profiling on." %
             (" --templates %d" % args.templates if args.templates > 0 else "", T, tbases / 1e9, len(rec), rows[0]["accepted"], rows[0]["columns"] / 1e9, threads, args.passes), "",
             "| call | wall per pass (s) | best vs the old entry point | strings to the host (GB) | table positions (M) | string kernels (ms) | `cns_table_tally` (ms) | `cns_table_finish` (ms) |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %+.3f s | %.2f | %.1f | %.1f | %.2f | %.2f |" % (r["label"], ", ".join("%.3f" % w for w in r["walls"]), min(r["walls"]) - base, r["string_bytes"] / 1e9,
                                                                               r["words"] / 1e6, r["strings_ms"], r["tally_ms"], r["finish_ms"]))
    rt = rows[2]
    lines += ["", "Tables of `STRINGS | TABLE` and `TABLE` are equal byte for byte: %s." % same, ""]
    if rt["tally_ms"] > 0:
        rate = rt["adds"] * 4 / (rt["tally_ms"] / 1e3)
        lines += ["`cns_table_tally`: %.3f G atomic adds of 4 bytes per pass (= the sum of all counts) in %.2f ms: **%.3f TB/s of added bytes**, %.0f %% of the %.1f TB/s "
                  "`MI355X_MICROARCH.md` gives for float adds in 256-byte wave-instructions; %.2f G columns read per pass, %.1f G columns/s."
                  % (rt["adds"] / 1e9, rt["tally_ms"], rate / 1e12, 100 * rate / ATOMIC_RATE_GUIDE, ATOMIC_RATE_GUIDE / 1e12, rt["columns"] / 1e9, rt["columns"] / 1e9 / (rt["tally_ms"] / 1e3)), ""]
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    vol.free()
    ctx.close()


if __name__ == "__main__":
    main()
