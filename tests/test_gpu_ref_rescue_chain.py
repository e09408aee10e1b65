"""mecat2ref's rescue stage on the device, the whole chain: seed -> extend -> mhip_ref_rescue_run* / _fetch (mecat_amd/csrc/ref_rescue.hip)
on reads with a deletion, an insert, an inverted middle, halves from two chromosomes or from a repeat copy, at -n 1, 2 and 10 and -b 1 and
10, both rounds, against the restatement tests/ref_rescue_ref.py (pinned to the unmodified functions by tests/test_ref_rescue_cpu.py):
the searches' candidates from restated segment records, their extension by tests/ref_ext_ref.py, the printed order, and the strings
rebuilt from the device's columns.  The reads are tests/ref_rescue_cases.py's chain_reads, made from ref_cand.npz's reference; the restatement runs once per setting."""
import os
import zlib

import numpy as np
import pytest

import ref_cand_cases as RC
import ref_cand_ref as R
import ref_ext_cases as XC
import ref_ext_ref as X
import ref_rescue_cases as SC
import ref_rescue_ref as S

pytestmark = pytest.mark.gpu

CUTOFF = 0.25
T = 6


@pytest.fixture(scope="module")
def dev():
    import mecat_amd.hip as M
    base = RC.fixture()
    ref_fasta = base["ref_fasta"].tobytes()
    codes, letters = XC.ref_codes(ref_fasta)
    reads = SC.fixture()["tool_reads"]          # (== SC.chain_reads(codes): tests/test_ref_rescue_cpu.py)
    ctx = M.Context(0)
    g = RC.RefGenome(ref_fasta)
    ref, idx = g.upload(ctx)
    pac, nplane, offs, nb = XC.pack_reads(reads)
    vol = M.Volume(ctx, pac, offs, nb, 0)
    M.volume_set_nplane(ctx, vol, nplane)
    d = dict(M=M, ctx=ctx, g=g, ref=ref, idx=idx, vol=vol, reads=reads, n=len(reads), codes=codes, index=R.Index(letters), pac=pac, nplane=nplane, offs=offs,
             dbs={}, ext={}, runs={})
    yield d
    idx.free(); ref.free(); vol.free(); g.free(); ctx.close()


def chain(dev, maxc, num_output, rnd, entry="host", env=None):
    """seed -> extend -> rescue on all reads -> dict(first=(res, offs, words), out=ref_rescue_fetch's dict, stats)"""
    M, ctx, n = dev["M"], dev["ctx"], dev["n"]
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        cands, cnt = M.ref_seed_reads(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, M.ref_seed_params(0, maxc=maxc, round=rnd))
        first = M.ref_extend(ctx, dev["ref"], dev["vol"], 0, n, maxc, cands, cnt)
        p = M.ref_rescue_params(0, maxc=maxc, round=rnd, num_output=num_output)
        if entry == "host":
            tot = M.ref_rescue_run(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, p, first[0])
        else:
            tot = M.ref_rescue_run_dev(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, p, None)
        out = M.ref_rescue_fetch(ctx, n, num_output, tot)
        return dict(first=first, cands=cands, out=out, stats=M.ref_rescue_stats(), again=M.ref_extend_fetch(ctx, n, maxc, len(first[2])))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def restated(dev, rid, rnd, first_rows, maxc, num_output):
    """the restatement for one read on the device's first results -> S.rescue_read's dict + the slots it prints"""
    read = dev["reads"][rid]
    L = len(read)

    def database(strand):
        key = (rid, rnd, strand)
        if key not in dev["dbs"]:
            dev["dbs"][key] = S.seed_records(dev["index"], R.revcomp(read) if strand else read, rnd, CUTOFF)
        return dev["dbs"][key]

    def extend(c):
        key = (rid, c["chain"], c["loc1"], c["loc2"])
        if key not in dev["ext"]:
            dev["ext"][key] = X.extend(dev["codes"], read, c["chain"], c["loc1"], c["loc2"])
        w = dev["ext"][key]
        return dict(w, chain=c["chain"], vscore=c["score"]) if w["ok"] else None
    ok = [s for s in range(maxc) if first_rows[s]["ok"]]
    first = [dict(qb=int(first_rows[s]["qb"]), qe=int(first_rows[s]["qe"]), chain=int(first_rows[s]["chain"]), sb=int(first_rows[s]["sb"]), se=int(first_rows[s]["se"])) for s in ok]
    w = S.rescue_read(first, L, num_output, database, extend, 2000 if rnd else 1000, len(dev["codes"]), 5 if rnd else min(20, 5 + L // 1000), CUTOFF)
    slot_of = {t: s for t, s in enumerate(ok)}
    nid = len(ok)
    for j, (_, _, _, r) in enumerate(w["tries"]):
        if r is not None:
            slot_of[nid] = maxc + j
            nid += 1
    w["slots"] = [slot_of[i] for i in w["printed"]]
    return w


def check(dev, run, maxc, num_output, rnd):
    """one run against the restatement, read by read -> counts of what was seen"""
    res, out = run["first"][0], run["out"]
    seen = dict(went_on=0, cands=0, ok=0, attached=0, unattached=0, no_ok_first=0, bytes=0)
    for rid in range(dev["n"]):
        w = restated(dev, rid, rnd, res[rid], maxc, num_output)
        assert out["out_slots"][rid, :out["out_counts"][rid]].tolist() == w["slots"], (rid, out["out_slots"][rid], w["slots"])
        assert (out["out_slots"][rid, out["out_counts"][rid]:] == -1).all()
        assert out["counts"][rid] == len(w["tries"]), (rid, out["counts"][rid], w["tries"])
        seen["went_on"] += int(w["go_on"])
        seen["no_ok_first"] += int(not res[rid]["ok"].any())
        for j, (owner, side, c, r) in enumerate(w["tries"]):
            g = out["cands"][rid, j]
            assert (int(g["loc1"]), int(g["loc2"]), int(g["score"]), int(g["chain"])) == (c["loc1"], c["loc2"], c["score"], c["chain"]), (rid, j)
            rr = out["res"][rid, j]
            want = X.extend(dev["codes"], dev["reads"][rid], c["chain"], c["loc1"], c["loc2"]) if r is None else r
            assert tuple(int(rr[k]) for k in XC.RES_FIELDS) == tuple(want[k] for k in XC.RES_FIELDS), (rid, j)
            s = rid * T + j
            words = out["words"][int(out["word_offs"][s]): int(out["word_offs"][s + 1])]
            seen["cands"] += 1
            if r is None:
                assert len(words) == 0
                continue
            assert (int(rr["chain"]), int(rr["vscore"])) == (c["chain"], c["score"])
            strs = XC.lib_strings(rr, words, dev["pac"], dev["nplane"], dev["offs"][rid, 0], dev["g"].pac)
            assert strs is not None and (zlib.crc32(strs[0]), zlib.crc32(strs[1])) == (zlib.crc32(r["qmap"]), zlib.crc32(r["smap"])), (rid, j)
            seen["ok"] += 1
        # the read's bytes of the result file: mecat_amd/host/ref_results.cpp on the two fetches == the restated records in printed order
        fo, ro = run["first"][1][rid * maxc: (rid + 1) * maxc + 1], out["word_offs"][rid * T: (rid + 1) * T + 1]
        got = SC.lib_read_records(rid, w["slots"], res[rid], fo, run["first"][2], out["res"][rid], ro, out["words"], dev["pac"], dev["nplane"], dev["offs"][rid, 0],
                                  dev["g"].pac)
        want = []
        for s in w["slots"]:
            if s < maxc:
                c = run["cands"][rid, s]
                key = (rid, int(c["chain"]), int(c["loc1"]), int(c["loc2"]))
                if key not in dev["ext"]:
                    dev["ext"][key] = X.extend(dev["codes"], dev["reads"][rid], key[1], key[2], key[3])
                r = dict(dev["ext"][key], chain=key[1], vscore=int(c["score"]))
            else:
                r = w["tries"][s - maxc][3]
            want.append(b"%d\t%c\t%d\t%d\t%d\t%d\t%d\t%d\n%s\n%s\n" % (rid, b"FR"[r["chain"]], r["vscore"], r["qb"], r["qe"], r["qs"], r["sb"], r["se"], r["qmap"], r["smap"]))
        assert got == b"".join(want), rid
        seen["bytes"] += len(got)
        att = sum(1 for a in w["after"] if a["parent_id"] != -1)
        seen["attached"] += att
        seen["unattached"] += sum(1 for t in w["tries"] if t[3] is not None) - att if w["go_on"] else 0
    st = run["stats"]
    assert (st["reads"], st["went_on"], st["candidates"]) == (dev["n"], seen["went_on"], seen["cands"]), (st, seen)
    return seen


def assert_same(a, b, what):
    for k in ("out_slots", "out_counts", "cands", "counts", "res", "word_offs", "words"):
        assert np.array_equal(a["out"][k], b["out"][k]), (what, k)


@pytest.fixture(scope="module")
def base_run(dev):
    return chain(dev, 2, 10, 0)


@pytest.mark.parametrize("maxc,num_output", [(1, 10), (2, 10), (2, 1), (10, 10), (10, 1)])
def test_chain_equals_the_restatement(dev, base_run, maxc, num_output):
    run = base_run if (maxc, num_output) == (2, 10) else chain(dev, maxc, num_output, 0)
    seen = check(dev, run, maxc, num_output, 0)
    if maxc <= 2:          # where the rescue finds what the list lacks
        assert seen["went_on"] >= 8 and seen["ok"] >= 4 and seen["attached"] >= 1 and seen["unattached"] >= 1, seen
    # the first extension is still there, unchanged
    for x, y in zip(run["first"], run["again"]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("maxc,num_output", SC.TOOL_RUNS)
def test_chain_equals_the_whole_tool(dev, base_run, maxc, num_output):
    """seed -> extend -> rescue against what the unmodified tool recorded for every read at this -n / -b: the results the rescue started
    from, the results it added (fields and the CRCs of the strings rebuilt from the device's columns), and the read's bytes of the result
    file as mecat_amd/host/ref_results.cpp writes them"""
    runs = {0: base_run if (maxc, num_output) == (2, 10) else chain(dev, maxc, num_output, 0)}
    all_calls = SC.fixture()["tool"][(maxc, num_output)]
    # the tool's flow: round 1 for every read, round 2 (2 000-base segments) for the reads whose round 1 left no entry
    assert sorted(c["read"] for c in all_calls if c["block_size"] == 1000) == list(range(dev["n"]))
    second = [c["read"] for c in all_calls if c["block_size"] == 2000]
    assert second == [c["read"] for c in all_calls if c["block_size"] == 1000 and not c["after"]] and len(second) >= 1
    runs[1] = chain(dev, maxc, num_output, 1)
    F = ("vscore", "chain", "qb", "qe", "qs", "sb", "se", "cols")
    added = 0
    for c in all_calls:
        rid = c["read"]
        run = runs[int(c["block_size"] == 2000)]
        res, out = run["first"][0], run["out"]

        def rows_of(rows, offs, words, base):
            got = []
            for k in range(len(rows)):
                if rows[k]["ok"]:
                    st = XC.lib_strings(rows[k], words[int(offs[base + k]): int(offs[base + k + 1])], dev["pac"], dev["nplane"], dev["offs"][rid, 0], dev["g"].pac)
                    assert st is not None
                    got.append([int(rows[k][f]) for f in F] + [zlib.crc32(st[0]), zlib.crc32(st[1])])
            return got
        assert rows_of(res[rid], run["first"][1], run["first"][2], rid * maxc) == c["results"][:c["nres0"]], rid
        assert rows_of(out["res"][rid, :out["counts"][rid]], out["word_offs"], out["words"], rid * T) == c["results"][c["nres0"]:], rid
        # the rescue candidates: every extend_candidate call the tool's rescue made for the read, in call order, and what it returned
        got = [(int(k["loc1"]), int(k["loc2"]), int(k["score"]), int(k["chain"]), int(r["ok"])) for k, r in zip(out["cands"][rid, :out["counts"][rid]], out["res"][rid])]
        assert got == c["extends"], (rid, got, c["extends"])
        added += c["nres1"] - c["nres0"]
        slots = out["out_slots"][rid, :out["out_counts"][rid]]
        text = SC.lib_read_records(rid, slots, res[rid], run["first"][1][rid * maxc: (rid + 1) * maxc + 1], run["first"][2], out["res"][rid],
                                   out["word_offs"][rid * T: (rid + 1) * T + 1], out["words"], dev["pac"], dev["nplane"], dev["offs"][rid, 0], dev["g"].pac)
        assert text is not None and (len(text), zlib.crc32(text), len(slots)) == (c["nbytes"], c["crc"], c["records"]), rid
    assert added >= 5


NEAR_FIRST, NEAR_LAST = 21, 22          # chain_reads(): the reads made next to the reference's first and last base


def hand_made_rows(dev, true_alns):
    """hand-made first lists on the fixture's reads -> per read [(qb, qe, chain, sb, se)] in list order.  true_alns[rid] = (qb, qe, chain,
    sb, se) of a real alignment of the read (or None): the first entry lies on its diagonal, so the read's own seeds are in the segments
    the searches scan, and one of its four ends is put, by the read's number, at the CLIPPED gate (2000 / 2001 on the read side, on the
    reference side where the entry lies about its place) or on / beside a segment boundary (where the scans start).  Two entries of
    equal length on the other strand follow (ties, the other strand's records), then four entries at the containment edges; short reads test 0.9 of the read at ceil and one below"""
    G = len(dev["codes"])
    out = []
    for rid, read in enumerate(dev["reads"]):
        L = len(read)
        t = true_alns[rid]
        if L < 6000 or t is None:
            full = -(-9 * L // 10)
            out.append([(0, full - (rid % 3 == 0), rid % 2, 40000, 40000 + full)])
            continue
        qb, qe, c, sb, se = t
        diag = lambda q: sb + (q - qb)
        q0, q1 = 2600, L - 2600
        s0, s1 = diag(q0), diag(q1)
        B0, B1 = s0 // 2000 * 2000, s1 // 2000 * 2000          # boundaries of both block sizes
        fam = rid % 12
        if fam in (0, 1):
            q0 = 2000 + fam
            s0 = diag(q0)
        elif fam in (2, 3):
            q1 = L - 2000 - (fam - 2)
            s1 = diag(q1)
        elif fam in (4, 5):
            s0 = 2000 + (fam - 4)
        elif fam in (6, 7):
            s1 = G - 2000 - (fam - 6)
        elif fam in (8, 9):
            s0 = B0 - (fam - 8)
        else:
            s1 = B1 - (fam - 10)
        if s0 >= s1:          # (an entry that lies about one end keeps its ends in order)
            s0, s1 = (s1 - 3000, s1) if fam in (6, 7, 10, 11) else (s0, s0 + 3000)
        rows = [(q0, q1, c, s0, s1), (2500, 4500, 1 - c, 20000, 22000), (2700, 4700, 1 - c, 50000, 52000)]
        # behind them the containment edges against the second entry, (2500, 4500, 1 - c, 20000, 22000): each comparison at equality
        # (removed) and one off it (kept)
        o = 1 - c
        rows += ([(2400, 4300, o, 20100, 21900), (2399, 4290, o, 20100, 21900), (2600, 4600, o, 20100, 21900), (2700, 4601, o, 20100, 21900)] if rid % 2 == 0 else
                 [(2600, 4400, o, 19900, 21900), (2600, 4390, o, 19899, 21900), (2600, 4380, o, 20100, 22100), (2600, 4370, o, 20100, 22101)])
        # the reference-side gates need seeds next to the reference's ends: the two reads that lie there carry both sides of the edge,
        # in two entries of which neither contains the other
        if rid == NEAR_FIRST:
            rows = [(2600, q1, c, 2001, diag(q1)), (2450, q1 - 160, c, 2000, diag(q1 - 160)), (2500, 3500, 1 - c, 20000, 21000)]
        elif rid == NEAR_LAST:
            rows = [(q0, q1, c, diag(q0), G - 2001), (q0 + 160, q1 + 150, c, diag(q0 + 160), G - 2000), (2500, 3500, 1 - c, 20000, 21000)]
        out.append(rows)
    return out


@pytest.mark.parametrize("rnd", [0, 1])
def test_hand_made_results_through_the_run(dev, base_run, rnd):
    """mhip_ref_rescue_run on hand-made result arrays: ref_rescue_find's gates, scan bounds and tie rule on the reads' own segment
    records against the restatement (seed_records + searches), the candidates' extension, and the printed slots"""
    M, ctx, n = dev["M"], dev["ctx"], dev["n"]
    maxc, num_output = 10, 10
    res = np.zeros((n, maxc), dtype=M.REF_RESULT_DTYPE)
    true_alns = []
    for rows in base_run["first"][0]:
        ok = [r for r in rows if r["ok"]]
        r = max(ok, key=lambda r: int(r["qe"]) - int(r["qb"])) if ok else None
        true_alns.append(None if r is None else (int(r["qb"]), int(r["qe"]), int(r["chain"]), int(r["sb"]), int(r["se"])))
    for rid, rows in enumerate(hand_made_rows(dev, true_alns)):
        for t, (qb, qe, c, sb, se) in enumerate(rows):
            r = res[rid, t + (t > 1)]          # (slot 2 stays empty: ids are not slots)
            r["ok"], r["qb"], r["qe"], r["chain"], r["sb"], r["se"], r["qs"], r["cols"], r["vscore"] = 1, qb, qe, c, sb, se, len(dev["reads"][rid]), qe - qb, 9
    p = M.ref_rescue_params(0, maxc=maxc, round=rnd, num_output=num_output)
    tot = M.ref_rescue_run(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, p, res)
    out = M.ref_rescue_fetch(ctx, n, num_output, tot)
    seen = dict(went_on=0, cands=0, left=0, right=0, early=0, removed=0, kept_at_edge=0)
    sides = {}
    for rid in range(n):
        w = restated(dev, rid, rnd, res[rid], maxc, num_output)
        assert out["counts"][rid] == len(w["tries"]), (rid, out["counts"][rid], [(o, s, k) for o, s, k, _ in w["tries"]])
        for j, (owner, side, k, r) in enumerate(w["tries"]):
            g = out["cands"][rid, j]
            assert (int(g["loc1"]), int(g["loc2"]), int(g["score"]), int(g["chain"])) == (k["loc1"], k["loc2"], k["score"], k["chain"]), (rid, j)
            want = dev["ext"][(rid, k["chain"], k["loc1"], k["loc2"])]
            assert tuple(int(out["res"][rid, j][f]) for f in XC.RES_FIELDS) == tuple(want[f] for f in XC.RES_FIELDS), (rid, j)
            seen["left" if side == 0 else "right"] += 1
        assert out["out_slots"][rid, :out["out_counts"][rid]].tolist() == w["slots"], (rid, out["out_slots"][rid], w["slots"])
        seen["went_on"] += int(w["go_on"])
        seen["early"] += int(not w["go_on"])
        seen["cands"] += len(w["tries"])
        nrows = int(res[rid]["ok"].sum())
        seen["removed"] += nrows - len(w["after"])
        seen["kept_at_edge"] += int(nrows == 7 and len(w["after"]) >= 5)
        sides[rid] = {(o, s_) for o, s_, _, _ in w["tries"]}
    st = M.ref_rescue_stats()
    assert (st["went_on"], st["candidates"]) == (seen["went_on"], seen["cands"])
    assert seen["early"] >= 1 and seen["left"] >= 3 and seen["right"] >= 3 and seen["removed"] >= 20 and seen["kept_at_edge"] >= 10, seen
    # the edges decide: qoff 2000 / 2001 (reads 12 / 13), L - qend 2000 / 2001 (14 / 15), soff and G - send 2001 / 2000 (entries 0 / 1)
    assert (0, 0) not in sides[12] and (0, 0) in sides[13] and (0, 1) not in sides[14] and (0, 1) in sides[15]
    assert (0, 0) in sides[NEAR_FIRST] and (1, 0) not in sides[NEAR_FIRST] and (0, 1) in sides[NEAR_LAST] and (1, 1) not in sides[NEAR_LAST]


def test_round_two(dev):
    run = chain(dev, 2, 10, 1)
    seen = check(dev, run, 2, 10, 1)
    assert seen["went_on"] >= 5 and seen["cands"] >= 3, seen


def test_device_resident_results_agree_with_the_host_array(dev, base_run):
    assert_same(chain(dev, 2, 10, 0, entry="dev"), base_run, "dev")
    M, ctx, n = dev["M"], dev["ctx"], dev["n"]
    # the last extension on this context has n x 2 slots: another list length is refused, and the context goes on working
    with pytest.raises(M.MhipError):
        M.ref_rescue_run_dev(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, M.ref_rescue_params(0, maxc=3), None)
    assert_same(chain(dev, 2, 10, 0), base_run, "after the refusal")


def test_second_launch_with_full_pools(dev, base_run):
    run = chain(dev, 2, 10, 0, env=dict(MECAT_REF_POOL="8"))
    assert run["stats"]["redone"] >= 1
    assert_same(run, base_run, "pool 8")


def test_small_column_budget(dev, base_run):
    run = chain(dev, 2, 10, 0, env=dict(MECAT_REF_COLS_BUDGET="3000"))
    assert dev["M"].ref_extend_stats()["slices"] > 1
    assert_same(run, base_run, "budget")
    for x, y in zip(run["first"], run["again"]):
        assert np.array_equal(x, y)


def test_refusals_leave_the_context_working(dev, base_run):
    M, ctx, n = dev["M"], dev["ctx"], dev["n"]
    res = base_run["first"][0]
    for kw in (dict(tech=1), dict(maxc=11), dict(maxc=0), dict(num_output=0), dict(round=2)):
        p = M.ref_rescue_params(**dict(dict(tech=0, maxc=2), **kw))
        with pytest.raises(M.MhipError):
            M.ref_rescue_run(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, p, np.zeros((n, p.maxc), dtype=M.REF_RESULT_DTYPE))
    with pytest.raises(M.MhipError):
        M.ref_rescue_run(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n + 1, M.ref_rescue_params(0, maxc=2), np.zeros((n + 1, 2), dtype=M.REF_RESULT_DTYPE))
    assert res.shape == (n, 2)
    # an index that was not built from this reference
    small = RC.RefGenome(RC.fasta_bytes([b"other"], [RC.letters(dev["codes"][:5000])], width=60))
    ref2, idx2 = small.upload(ctx)
    with pytest.raises(M.MhipError):
        M.ref_rescue_run(ctx, idx2, dev["ref"], dev["vol"], 0, n, M.ref_rescue_params(0, maxc=2), res)
    idx2.free(); ref2.free(); small.free()
    # a read of 100 000 letters (the tool's read buffers end there)
    pac, nplane, offs, nb = XC.pack_reads([np.full(100000, ord("A"), dtype=np.uint8)])
    long_vol = M.Volume(ctx, pac, offs, nb, 0)
    with pytest.raises(M.MhipError):
        M.ref_rescue_run(ctx, dev["idx"], dev["ref"], long_vol, 0, 1, M.ref_rescue_params(0, maxc=2), np.zeros((1, 2), dtype=M.REF_RESULT_DTYPE))
    long_vol.free()
    assert_same(chain(dev, 2, 10, 0), base_run, "after the refusals")
