#!/usr/bin/env python3
"""Golden vectors for the consensus table of mecat2cns (mecat_amd/csrc/cns_table.hip; mhip_cns_accept_templates_ex, mhip_debug_cns_table):
what the UNMODIFIED reference makes of it, through oracle/_ref/libref_cns_table.so (oracle/ref_harness_cns_table.cpp: mecat2cns compiled
from /root/reference/src, mecat_correction.cpp included where it lies).  Build container only:
    python tests/golden/make_golden_cns_table.py
Writes tests/golden/cns_table.npz, recorded results only:

  pipeline   for every template of both sets of cns_accept.npz (same parameters, same candidates, read from that file): a SHA-256 over the
             read_size CnsTableItems that consensus_one_read_can_* left in ConsensusThreadData::cns_table ({name}_table_sha) and one over the
             ident bytes identify_one_consensus_item gives them ({name}_ident_sha; "" for a template without candidates); for the first 8
             templates of each set the arrays themselves ({name}_table8 as [4, n] byte planes base / mat / ins / del, {name}_ident8,
             {name}_begin8).  The accepted (soff, send, aln_size) and string hashes seen here are asserted equal to cns_accept.npz's.
  sweep      sweep_ident: identify_one_consensus_item for every (mat, ins, del) with mat + ins <= 100 (MAX_CNS_OVLPS) and del <= mat + ins,
             348 551 triples in the order of cns_table_ref.sweep_triples (cov ascending, mat ascending, del ascending)
  adversarial pairs   meap_add_one_aln on a fresh table for the 700 gap-normalised outputs of pushgaps.npz (the reference's own
             normalize_gaps results; strings stay in that file, adv_pushgaps_sha ties them) and for GENERATED pairs of 1 - 300 columns drawn
             from the four column kinds with long template-gap runs: runs that begin with double gaps, runs of double gaps only, runs at the
             first and at the last column, runs at soff == 0, pairs without any template base (adv_gen_q / _s / _lens hold their strings).
             adv_soff, adv_tmpl_len per pair; adv_table: tmpl_len + 2 items per pair as [4, n] planes, the first and last item of each pair
             being the harness's guards (the reference's index -1 and tmpl_len)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cns_table_golden as TG  # noqa: E402
import cns_table_ref as R  # noqa: E402
import helpers as H  # noqa: E402

STORED = 8
MATCH, QGAP, SGAP, BOTH = 0, 1, 2, 3          # column kinds: q == s / '-' over a base / a base over '-' / '-' over '-'
LET = np.frombuffer(b"ACGT", dtype=np.uint8)


def strings_of(ops, rng):
    ops = np.asarray(ops)
    n = len(ops)
    s = np.where((ops == MATCH) | (ops == QGAP), LET[rng.integers(0, 4, n)], R.GAP).astype(np.uint8)
    q = np.where(ops == MATCH, s, np.where(ops == SGAP, LET[rng.integers(0, 4, n)], R.GAP)).astype(np.uint8)
    return q, s


def run_of(rng, kind, longest):
    """a run of template-gap columns: 0 query bases only, 1 begins with double gaps, 2 double gaps only, 3 mixed"""
    k = int(rng.integers(1, longest + 1))
    if kind == 0:
        return np.full(k, SGAP)
    if kind == 1:
        d = int(rng.integers(1, k + 1))
        return np.concatenate([np.full(d, BOTH), rng.choice([SGAP, BOTH], k - d, p=[0.7, 0.3]), [SGAP]]).astype(np.int64)
    if kind == 2:
        return np.full(k, BOTH)
    return rng.choice([SGAP, BOTH], k)


def generated_pairs(seed=41, count=360):
    """-> list of (q, s, soff, tmpl_len)"""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(count):
        mode = it % 9
        n = [1, 2, 3, 5, 64, 65, 129, 300][it // 9 % 8] if it % 2 else int(rng.integers(1, 301))
        body = []
        while sum(len(b) for b in body) < n:
            u = rng.random()
            if u < 0.25:
                body.append(run_of(rng, int(rng.integers(0, 4)), int(rng.choice([3, 20, 150]))))
            else:
                body.append(rng.choice([MATCH, QGAP], int(rng.integers(1, 12)), p=[0.8, 0.2]))
        ops = np.concatenate(body)[:n]
        soff = int(rng.integers(1, 6))
        if mode in (1, 2, 3, 4):            # a run at the first column: query bases / begins with double gaps / double gaps only / mixed
            r = run_of(rng, mode - 1, min(n, int(rng.choice([2, 10, 80]))))[:n]
            ops[: len(r)] = r
            if it % 4 < 2:
                soff = 0                    # ... in front of the first template base of the template: the reference counts at index -1
        elif mode == 5:                     # a run at the last column
            r = run_of(rng, int(rng.integers(0, 4)), min(n, int(rng.choice([2, 10, 80]))))[:n]
            ops[n - len(r):] = r
        elif mode == 6:                     # nothing but template gaps
            ops = run_of(rng, int(rng.integers(0, 4)), n)[:n]
            soff = int(rng.integers(0, 3))
        elif mode == 7:
            soff = 0
        q, s = strings_of(ops, rng)
        span = int((s != R.GAP).sum())
        tmpl_len = max(1, soff + span + int(rng.integers(0, 3)))
        out.append((q, s, soff, tmpl_len))
    return out


def main():
    out = {}
    A = np.load(os.path.join(H.GOLDEN, "cns_accept.npz"))
    for name in ("pacbio", "nanopore"):
        n = int(A[name + "_par"][0])
        res = TG.reference_tables(name, n)
        first = np.concatenate([[0], np.cumsum(A[name + "_nacc"])])
        tsha, isha = [], []
        for t, r in enumerate(res):
            if r is None:
                assert A[name + "_nacc"][t] == 0
                tsha.append(""); isha.append("")
                continue
            meta, sha, table, ident = r
            assert np.array_equal(meta, A[name + "_meta"][first[t]: first[t + 1]]) and sha == str(A[name + "_sha"][t]), (name, t)
            tsha.append(hashlib.sha256(table.tobytes()).hexdigest())
            isha.append(hashlib.sha256(ident.tobytes()).hexdigest())
        assert all(r is not None for r in res[:STORED])
        out[name + "_table_sha"], out[name + "_ident_sha"] = np.array(tsha), np.array(isha)
        out[name + "_table8"] = np.ascontiguousarray(np.concatenate([r[2] for r in res[:STORED]]).view(np.uint8).reshape(-1, 4).T)
        out[name + "_ident8"] = np.concatenate([r[3] for r in res[:STORED]])
        out[name + "_begin8"] = np.concatenate([[0], np.cumsum([len(r[2]) for r in res[:STORED]])]).astype(np.int64)
        print(name, "templates", n, "with a table", sum(r is not None for r in res), file=sys.stderr)
    out["sweep_ident"] = TG.reference_sweep()
    assert len(out["sweep_ident"]) == 348551
    pg = np.load(os.path.join(H.GOLDEN, "pushgaps.npz"))
    out["adv_pushgaps_sha"] = np.array(hashlib.sha256(pg["qout"].tobytes() + pg["tout"].tobytes()).hexdigest())
    cb = np.concatenate([[0], np.cumsum(pg["lens"].astype(np.int64))])
    rng = np.random.default_rng(40)
    pairs = []
    for i in range(len(pg["lens"])):
        q, s = pg["qout"][cb[i]: cb[i + 1]], pg["tout"][cb[i]: cb[i + 1]]
        soff = 0 if i % 4 == 0 else int(rng.integers(1, 5))
        pairs.append((q, s, soff, max(1, soff + int((s != R.GAP).sum()) + int(rng.integers(0, 3)))))
    gen = generated_pairs()
    pairs += gen
    tables = [TG.reference_add_one(*p) for p in pairs]
    out["adv_gen_lens"] = np.array([len(p[0]) for p in gen], dtype=np.int32)
    out["adv_gen_q"], out["adv_gen_s"] = np.concatenate([p[0] for p in gen]), np.concatenate([p[1] for p in gen])
    out["adv_soff"] = np.array([p[2] for p in pairs], dtype=np.int32)
    out["adv_tmpl_len"] = np.array([p[3] for p in pairs], dtype=np.int32)
    out["adv_table"] = np.ascontiguousarray(np.concatenate(tables).view(np.uint8).reshape(-1, 4).T)
    lead = [TG.leading_run(p[0], p[1]) for p in pairs]
    print("pairs %d (generated %d), leading run at soff == 0: %d, of them with a stray count at index -1: %d" % (
        len(pairs), len(gen), sum(1 for p, l in zip(pairs, lead) if l[0] and p[2] == 0), sum(1 for t in tables if t[0]["del_cnt"])), file=sys.stderr)
    path = os.path.join(H.GOLDEN, "cns_table.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path), file=sys.stderr)


if __name__ == "__main__":
    main()
