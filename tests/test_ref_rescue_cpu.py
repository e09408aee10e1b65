"""mecat2ref's rescue stage without a device: the restatement tests/ref_rescue_ref.py against what the UNMODIFIED rescue_clipped_align and
output_results recorded on the hand-made cases of tests/ref_rescue_cases.py (tests/golden/ref_rescue.npz,
tests/golden/make_golden_ref_rescue.py), and the exports of the stage's ABI."""
import zlib

import numpy as np
import pytest

import ref_cand_cases as RC
import ref_cand_ref as R
import ref_ext_cases as XC
import ref_ext_ref as X
import ref_rescue_cases as SC
import ref_rescue_ref as S

CUTOFF = 0.25


@pytest.fixture(scope="module")
def fx():
    return SC.fixture()


def restate(fx, c):
    """one case through the restatement -> (entries after, results after, the results added, printed ids)"""
    qs = len(c["read"])
    v, go_on = S.prep([S.entry(*e, t) for t, e in enumerate(c["entries"])], qs)
    tries, new = [], []
    if go_on:
        for owner, side, cand in S.searches(v, (c["fwd"], c["rev"]), c["block_size"], qs, len(fx["ref_codes"]), c["bc"], CUTOFF):
            w = X.extend(fx["ref_codes"], c["read"], cand["chain"], cand["loc1"], cand["loc2"])
            r = None
            if w["ok"]:
                r = dict(w, chain=cand["chain"], vscore=cand["score"])
                new.append(r)
            tries.append((owner, side, r))
    after, nres = S.finish(v, go_on, len(c["entries"]), qs, tries)
    return after, nres, new, S.output_ids(after, c["num_output"])


def test_fixture_holds_the_cases_it_was_made_for(fx):
    shown = fx["asserted"]
    assert shown["cases"] == len(fx["cases"]) >= 40
    for k in ("early_return", "left_attach", "right_attach", "ok_unattached", "no_location", "score2_gate", "gate_read_side", "gate_ref_side", "score2_over_20",
              "rescue_on_R", "rescue_round2", "containment_removals", "fourth_not_rescued", "num_output_cuts", "full_cut"):
        assert shown[k] >= 1, k
    assert shown["tie_winner_by_vscore"] == [7, 8, 7, 5]
    # the inputs are the ones tests/ref_rescue_cases.py makes today
    made = SC.make_cases(fx["ref_letters"])
    assert [m["name"] for m in made] == [c["name"] for c in fx["cases"]]
    for m, c in zip(made, fx["cases"]):
        assert np.array_equal(m["read"], c["read"]) and m["entries"] == c["entries"] and (m["block_size"], m["bc"], m["num_output"]) == (c["block_size"], c["bc"], c["num_output"])
        for k in ("fwd", "rev"):
            assert {s: (v[0], list(v[1]), list(v[2])) for s, v in m[k].items()} == {s: (v[0], list(v[1]), list(v[2])) for s, v in c[k].items()}, (c["name"], k)


def test_restatement_equals_the_tool(fx):
    for c in fx["cases"]:
        after, nres, new, printed = restate(fx, c)
        got = [[a[f] for f in SC.AFTER_FIELDS] for a in after]
        assert got == c["after"].tolist(), (c["name"], got, c["after"].tolist())
        assert nres == c["nresults"], c["name"]
        assert printed == c["printed"], (c["name"], printed, c["printed"])
        assert len(new) == len(c["new"]), c["name"]
        for r, want in zip(new, c["new"].tolist()):
            assert [r["vscore"], r["chain"], r["qb"], r["qe"], r["qs"], r["sb"], r["se"], r["cols"], zlib.crc32(r["qmap"]), zlib.crc32(r["smap"])] == want, c["name"]


def test_sort_keeps_the_order_of_equal_lengths(fx):
    c = next(c for c in fx["cases"] if c["name"] == "ties10")
    ids = c["after"][:, SC.AFTER_FIELDS.index("id")].tolist()
    assert ids == [0, 2, 5, 9, 3, 6, 1, 4, 8, 7] == c["printed"]


def test_restatement_equals_the_whole_tool(fx):
    """every call of rescue_clipped_align / output_results the unmodified tool made on the chain reads at -n 1, 2, 10 and -b 1, 10: the
    first list restated (candidates + extension) equals the results the call started from, the restated rescue equals the array and
    the results it left, and the restated records are the bytes the tool wrote for the read.  No recorded read is skipped."""
    reads = fx["tool_reads"]
    made = SC.chain_reads(fx["ref_codes"])
    assert len(made) == len(reads) and all(np.array_equal(a, b) for a, b in zip(made, reads))
    idx = R.Index(fx["ref_letters"])
    dbs, ext, lists = {}, {}, {}
    G = len(fx["ref_codes"])

    def extend_of(rid, chain, loc1, loc2):
        key = (rid, chain, loc1, loc2)
        if key not in ext:
            ext[key] = X.extend(fx["ref_codes"], reads[rid], chain, loc1, loc2)
        return ext[key]
    fields = lambda r: [r["vscore"], r["chain"], r["qb"], r["qe"], r["qs"], r["sb"], r["se"], r["cols"], zlib.crc32(r["qmap"]), zlib.crc32(r["smap"])]
    seen, empty_after_round1, rounds = set(), set(), [0, 0]
    for (n, b), calls in fx["tool"].items():
        for c in calls:
            rid, read = c["read"], reads[c["read"]]
            seen.add(rid)
            rnd = int(c["block_size"] == 2000)          # round 2 follows a round 1 that left no entry
            assert c["block_size"] == (2000 if rnd else 1000) and c["read_len"] == len(read) and c["bc"] == (5 if rnd else min(20, 5 + len(read) // 1000))
            assert rnd == int((n, b, rid) in empty_after_round1)
            if (rid, n, rnd) not in lists:
                lists[(rid, n, rnd)] = [dict(extend_of(rid, int(k[9]), int(k[0]), int(k[1])), chain=int(k[9]), vscore=int(k[6]))
                                        for k in R.candidates(idx, read, rnd, CUTOFF, n)]
            first = [r for r in lists[(rid, n, rnd)] if r["ok"]]
            assert [fields(r) for r in first] == c["results"][:c["nres0"]] and c["naln0"] == c["nres0"], (n, b, rid)
            assert c["before"] == [[r["qb"], r["qe"], r["chain"], r["sb"], r["se"], t] for t, r in enumerate(first)]

            def database(s):
                if (rid, s, rnd) not in dbs:
                    dbs[(rid, s, rnd)] = S.seed_records(idx, R.revcomp(read) if s else read, rnd, CUTOFF)
                return dbs[(rid, s, rnd)]

            def extend(k):
                w = extend_of(rid, k["chain"], k["loc1"], k["loc2"])
                return dict(w, chain=k["chain"], vscore=k["score"]) if w["ok"] else None
            w = S.rescue_read(first, len(read), b, database, extend, c["block_size"], G, c["bc"], CUTOFF)
            if not rnd and not w["after"]:
                empty_after_round1.add((n, b, rid))
            rounds[rnd] += 1
            assert [[a[f] for f in SC.AFTER_FIELDS] for a in w["after"]] == c["after"], (n, b, rid)
            # every extend_candidate call the rescue made: the candidate and whether it gave a result; every search that gave none
            assert [(k["loc1"], k["loc2"], k["score"], k["chain"], int(r is not None)) for _, _, k, r in w["tries"]] == c["extends"], (n, b, rid)
            assert sum(1 for x in c["finds"] if x[6]) == len(w["tries"]) and (w["go_on"] or not c["finds"]), (n, b, rid)
            new = [t[3] for t in w["tries"] if t[3] is not None]
            assert w["nresults"] == c["nres1"] and [fields(r) for r in new] == c["results"][c["nres0"]:], (n, b, rid)
            by_id = first + new
            text = b"".join(record_bytes(rid, by_id[i]) for i in w["printed"])
            assert (len(text), zlib.crc32(text), len(w["printed"])) == (c["nbytes"], c["crc"], c["records"]), (n, b, rid)
    assert seen == set(range(len(reads))) and rounds[1] >= 1 and rounds[0] == len(reads) * len(SC.TOOL_RUNS)


def record_bytes(rid, r):
    return b"%d\t%c\t%d\t%d\t%d\t%d\t%d\t%d\n%s\n%s\n" % (rid, b"FR"[r["chain"]], r["vscore"], r["qb"], r["qe"], r["qs"], r["sb"], r["se"], r["qmap"], r["smap"])


def test_host_records_are_the_result_file_bytes(fx):
    """ref_read_records on restated results (first list at -n 1, the rescue's) == the records in output_results' order"""
    from mecat_amd import hip
    base = RC.fixture()
    reads = SC.chain_reads(fx["ref_codes"])
    idx = R.Index(fx["ref_letters"])
    g = RC.RefGenome(base["ref_fasta"].tobytes())
    pac, npl, offs, _ = XC.pack_reads(reads)
    maxc, attached, refused = 2, 0, 0
    for rid in range(9, 15):
        read = reads[rid]
        L = len(read)
        first = []
        for c in R.candidates(idx, read, 0, CUTOFF, 1):
            w = X.extend(fx["ref_codes"], read, int(c[9]), int(c[0]), int(c[1]))
            first.append(dict(w, chain=int(c[9]), vscore=int(c[6])))
        ok = [r for r in first if r["ok"]]

        def extend(c):
            w = X.extend(fx["ref_codes"], read, c["chain"], c["loc1"], c["loc2"])
            return dict(w, chain=c["chain"], vscore=c["score"]) if w["ok"] else None
        w = S.rescue_read(ok, L, 10, lambda s: S.seed_records(idx, R.revcomp(read) if s else read, 0, CUTOFF), extend, 1000, len(fx["ref_codes"]),
                          min(20, 5 + L // 1000), CUTOFF)
        found = [t[3] for t in w["tries"]]
        by_id = ok + [r for r in found if r is not None]
        attached += sum(1 for a in w["after"] if a["parent_id"] != -1)

        def rows(results, n):          # one set as the device hands it over: rows, word offsets, words
            res = np.zeros(n, dtype=hip.REF_RESULT_DTYPE)
            words, o = [], [0]
            for k, r in enumerate(results):
                if r is not None and r["ok"]:
                    for f in XC.RES_FIELDS:
                        res[k][f] = r[f]
                    res[k]["chain"], res[k]["vscore"] = r["chain"], r["vscore"]
                    words.append(X.columns_of(r["qmap"], r["smap"]))
                o.append(o[-1] + (len(words[-1]) if r is not None and r["ok"] else 0))
            o += [o[-1]] * (n - len(results))
            return res, np.array(o, dtype=np.uint64), np.concatenate(words) if words else np.zeros(0, dtype=np.uint32)
        # the ok results lie in the list's first slots here; rescue slot j = the j-th try
        slot_of, nid = {t: t for t in range(len(ok))}, len(ok)
        for j, r in enumerate(found):
            if r is not None:
                slot_of[nid] = maxc + j
                nid += 1
        slots = [slot_of[i] for i in w["printed"]]
        a, b = rows(ok, maxc), rows(found, 6)
        got = SC.lib_read_records(rid, slots, a[0], a[1], a[2], b[0], b[1], b[2], pac, npl, offs[rid, 0], g.pac)
        assert got == b"".join(record_bytes(rid, by_id[i]) for i in w["printed"]), rid
        if len(ok) < maxc:          # a slot that holds no ok result is refused
            assert SC.lib_read_records(rid, [len(ok)], a[0], a[1], a[2], b[0], b[1], b[2], pac, npl, offs[rid, 0], g.pac) is None
            refused += 1
    assert attached >= 2 and refused >= 1
    g.free()


def test_abi_exports():
    """fails before the stage existed: the entry points are missing"""
    from mecat_amd import hip
    import mecat_amd
    L = hip.lib()
    for name in ("mhip_ref_rescue_params_default", "mhip_ref_rescue_run", "mhip_ref_rescue_run_dev", "mhip_ref_rescue_fetch", "mhip_ref_rescue_stats",
                 "mhip_debug_ref_rescue_prep", "mhip_debug_ref_rescue_finish"):
        assert hasattr(L, name), name
    p = mecat_amd.ref_rescue_params(0)
    assert (p.maxc, p.round, p.num_output, p.tech, p.ddfs_cutoff) == (10, 0, 10, 0, 0.25)
    assert mecat_amd.ref_rescue_params(0, num_output=2).num_output == 2 and isinstance(p, mecat_amd.RefRescueParams)
    assert all(callable(getattr(mecat_amd, n)) for n in ("ref_rescue_run", "ref_rescue_run_dev", "ref_rescue_fetch"))
