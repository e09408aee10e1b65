"""mecat2ref in nanopore mode on the device, the whole chain: seed (-x 1) -> mhip_ref_xextend_run -> mhip_ref_xrescue_run* -> the two
fetches -> ref_read_records, against what the whole unmodified tool recorded at `-x 1` with -n 10 -b 10 and -n 2 -b 1
(tests/golden/ref_xext.npz: tool_x_*): the results the rescue started from, the rescue candidates it extended and what came of them,
the results it added, and the read's bytes of the result file.  The reads are the PacBio chain's (tests/ref_rescue_cases.py) and the
fixture's extra ones, which are the ones that attach under X-drop (tests/ref_xext_cases.py: extra_chain_reads)."""
import zlib

import numpy as np
import pytest

import ref_cand_cases as RC
import ref_ext_cases as XC
import ref_rescue_cases as SC
import ref_xext_cases as XX

pytestmark = pytest.mark.gpu
T = 6


@pytest.fixture(scope="module")
def dev():
    import mecat_amd.hip as M
    base = RC.fixture()
    ref_fasta = base["ref_fasta"].tobytes()
    reads = XX.chain_reads()
    ctx = M.Context(0)
    g = RC.RefGenome(ref_fasta)
    ref, idx = g.upload(ctx)
    pac, nplane, offs, nb = XC.pack_reads(reads)
    vol = M.Volume(ctx, pac, offs, nb, 0)
    M.volume_set_nplane(ctx, vol, nplane)
    yield dict(M=M, ctx=ctx, g=g, ref=ref, idx=idx, vol=vol, reads=reads, n=len(reads), pac=pac, nplane=nplane, offs=offs)
    idx.free(); ref.free(); vol.free(); g.free(); ctx.close()


def chain(dev, maxc, num_output, rnd, entry="host"):
    """seed -> x-extend -> x-rescue on all reads -> dict(first=(res, offs, words), out=ref_rescue_fetch's dict)"""
    M, ctx, n = dev["M"], dev["ctx"], dev["n"]
    cands, cnt = M.ref_seed_reads(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, M.ref_seed_params(1, maxc=maxc, round=rnd))
    first = M.ref_xextend(ctx, dev["ref"], dev["vol"], 0, n, maxc, cands, cnt)
    p = M.ref_rescue_params(1, maxc=maxc, round=rnd, num_output=num_output)
    if entry == "host":
        tot = M.ref_xrescue_run(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, p, first[0])
    else:
        tot = M.ref_xrescue_run_dev(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, p, None)
    out = M.ref_rescue_fetch(ctx, n, num_output, tot)
    return dict(first=first, out=out, again=M.ref_extend_fetch(ctx, n, maxc, len(first[2])))


@pytest.mark.parametrize("maxc,num_output", XX.TOOL_RUNS)
def test_chain_equals_the_whole_tool(dev, maxc, num_output):
    all_calls = XX.fixture()["tool"][(maxc, num_output)]
    # the tool's flow: round 1 for every read, round 2 (2 000-base segments) for the reads whose round 1 left no entry
    assert sorted(c["read"] for c in all_calls if c["block_size"] == 1000) == list(range(dev["n"]))
    second = [c["read"] for c in all_calls if c["block_size"] == 2000]
    assert second == [c["read"] for c in all_calls if c["block_size"] == 1000 and not c["after"]] and len(second) >= 1
    runs = {0: chain(dev, maxc, num_output, 0), 1: chain(dev, maxc, num_output, 1, entry="dev")}
    F = ("vscore", "chain", "qb", "qe", "qs", "sb", "se", "cols")
    seen = dict(added=0, early=0, left=0, right=0, not_attached=0, nbytes=0)
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
        slots = out["out_slots"][rid, :out["out_counts"][rid]]
        text = SC.lib_read_records(rid, slots, res[rid], run["first"][1][rid * maxc: (rid + 1) * maxc + 1], run["first"][2], out["res"][rid],
                                   out["word_offs"][rid * T: (rid + 1) * T + 1], out["words"], dev["pac"], dev["nplane"], dev["offs"][rid, 0], dev["g"].pac)
        assert text is not None and (len(text), zlib.crc32(text), len(slots)) == (c["nbytes"], c["crc"], c["records"]), rid
        att = sum(1 for a in c["after"] if a[8] != -1)
        seen["added"] += c["nres1"] - c["nres0"]
        seen["early"] += int(bool(c["after"]) and not c["finds"])
        seen["left"] += sum(1 for a in c["after"] if a[6] != -1)
        seen["right"] += sum(1 for a in c["after"] if a[7] != -1)
        seen["not_attached"] += max(0, len(c["extends"]) - att)
        seen["nbytes"] += len(text)
    assert seen["added"] >= 5 and seen["early"] >= 1 and seen["left"] >= 1 and seen["right"] >= 1 and seen["not_attached"] >= 1 and seen["nbytes"] > 100000, seen
    # the first extension is still there, unchanged
    for run in runs.values():
        for x, y in zip(run["first"], run["again"]):
            assert np.array_equal(x, y)


def test_the_technologies_keep_to_their_entry_points(dev):
    M, ctx, n = dev["M"], dev["ctx"], dev["n"]
    before = chain(dev, 2, 1, 0)
    zero = np.zeros((n, 2), dtype=M.REF_RESULT_DTYPE)
    with pytest.raises(M.MhipError, match="nanopore"):          # the PacBio call still refuses tech = 1, and names the other call
        M.ref_rescue_run(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, M.ref_rescue_params(1, maxc=2), zero)
    with pytest.raises(M.MhipError, match="PacBio"):
        M.ref_xrescue_run(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, M.ref_rescue_params(0, maxc=2), zero)
    # the PacBio calls' other refusals
    for kw in (dict(maxc=11), dict(maxc=0), dict(num_output=0), dict(round=2)):
        p = M.ref_rescue_params(**dict(dict(tech=1, maxc=2), **kw))
        with pytest.raises(M.MhipError):
            M.ref_xrescue_run(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, p, np.zeros((n, p.maxc), dtype=M.REF_RESULT_DTYPE))
    with pytest.raises(M.MhipError):          # the last extension on this context has n x 2 slots
        M.ref_xrescue_run_dev(ctx, dev["idx"], dev["ref"], dev["vol"], 0, n, M.ref_rescue_params(1, maxc=3), None)
    after = chain(dev, 2, 1, 0)
    for k in ("out_slots", "out_counts", "cands", "counts", "res", "word_offs", "words"):
        assert np.array_equal(before["out"][k], after["out"][k]), k
