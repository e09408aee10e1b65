"""mhip_ref_xextend_run on the pairs of tests/xd_edge_cases.py (families A, B, C and E as tests/test_xd_edge_cases_cpu.py proves them):
here every gap column the block's traceback reports ends up in the result, so the column sink is what is checked — the gap behind a run
(sink.gap(T.n, ..)), the lean loop's own count of it, and the claim that a ring block that outgrows its window leaves the sink empty for
the wide redo.  Fields against orc_xdrop_go on extract_sequences' window, the rebuilt strings byte for byte against the strings of the
walker over the oracle's blocks, the `redone` stat against the walker's count, and MECAT_XD_WIDE=1 against the default."""
import os

import pytest

import ref_xext_cases as XX
import xd_edge_cases as E
from test_gpu_ref_xextend import FIELDS, Side, assert_same_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import mecat_amd.hip as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["A", "B", "C/0", "C/1", "C/2", "C/3", "E"])          # (C in quarters: a few seconds each; every job is in one)
def test_edge_pairs_fields_strings_and_redone_blocks(ctx, name):
    import mecat_amd.hip as M
    v = E.ref_view(name)
    cands, walks = v["cands"], v["walks"]
    # the walker is XdropAligner::go on this view's windows: its fields are orc_xdrop_go's
    want = [XX.xgo(v["codes"], v["reads"][int(c[0])], int(c[1]), int(c[2]), int(c[3])) for c in cands]
    for c, w, x in zip(cands, walks, want):
        r = w["res"]
        assert (r["query_start"], r["query_end"], w["sb"] + r["target_start"], w["sb"] + r["target_end"], r["columns"], r["matches"]) == \
               (x["qb"], x["qe"], x["sb"], x["se"], x["cols"], x["matches"]), c
    blocks = [b for w in walks for b in w["left"] + w["right"]]
    redone = sum(b["widest"] > E.RING_CELLS for b in blocks)
    n_ok = sum(x["ok"] for x in want)
    print("family %s through ref_xextend: %d candidates, %d ok, %d blocks, %d outgrow the ring" % (name, len(cands), n_ok, len(blocks), redone))
    # Every candidate whose span passes 1 000 has its strings compared below, and that is all of them but the ones named here: family C's
    # trim edges whose block 1 is refused or has no run (nothing is kept, the half is empty), and family E's k = 86 pairs from the start
    # point 400 bases before the reads' end, whose left half stops 18 bases into its second block (a span of 913).
    short = sorted((lab for lab, x in zip(v["labels"], want) if not x["ok"]), key=str)
    if name == "C/3":
        assert short == sorted([("trim", d, r) for d in (0, 1, None) for r in (0, 1) for _ in (0, 1)], key=str), short
    elif name == "E":
        assert short == sorted([("left", 86, front) for front in (700, 1000, 1300) for _ in (0, 1)], key=str), short
    else:
        assert not short, short
    if name == "A":          # both sides of the ring's limit are still there in this view
        assert {126, 127} <= set(b["widest"] for b in blocks)
    if name in "ABE":
        assert redone >= 50
    else:
        assert redone == 0
    sd = Side(M, ctx, v["text"], v["reads"], cands)
    try:
        got = sd.run()
        st = M.ref_xextend_stats()
        res, woffs, words = got
        flat = res.reshape(-1)
        bad = []
        for i, (w, x, s) in enumerate(zip(walks, want, sd.slot)):
            r = flat[int(s)]
            if tuple(int(r[k]) for k in FIELDS) != tuple(x[k] for k in FIELDS):
                bad.append((i, tuple(cands[i]), tuple(int(r[k]) for k in FIELDS), tuple(x[k] for k in FIELDS)))
                continue
            if not x["ok"]:
                assert woffs[s] == woffs[s + 1]
                continue
            strs = sd.strings(int(cands[i][0]), r, words[int(woffs[s]): int(woffs[s + 1])])
            assert strs is not None, (i, cands[i])          # (the bases in the strings equal the spans)
            qmap, smap = E.strings(w)
            if strs != (qmap, smap):
                k = next((j for j in range(min(len(qmap), len(strs[0]))) if (strs[0][j], strs[1][j]) != (qmap[j], smap[j])), -1)
                bad.append((i, tuple(cands[i]), "strings differ from column %d of %d" % (k, len(qmap)), strs[0][max(k - 8, 0): k + 8], qmap[max(k - 8, 0): k + 8],
                            strs[1][max(k - 8, 0): k + 8], smap[max(k - 8, 0): k + 8]))
        assert not bad, "%d of %d candidates differ: %s" % (len(bad), len(cands), bad[:3])
        assert st["redone"] == redone, st
        os.environ["MECAT_XD_WIDE"] = "1"
        try:
            wide = sd.run()
        finally:
            del os.environ["MECAT_XD_WIDE"]
        assert_same_run(wide, got, "all wide")
        assert M.ref_xextend_stats()["redone"] == 0
    finally:
        sd.free()
