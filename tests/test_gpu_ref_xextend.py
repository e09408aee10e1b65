"""mecat2ref on the device, stage 2 in nanopore mode: mhip_ref_xextend_run / _run_dev (mecat_amd/csrc/ref_xextend.hip, fetched by
mhip_ref_extend_fetch) against what the UNMODIFIED extend_candidate recorded with an XdropAligner (tests/golden/ref_xext.npz,
tests/golden/make_golden_ref_xext.py) and, beyond the fixture, against oracle/liboracle.so's orc_xdrop_go, which
tests/test_ref_xext_cpu.py pins to the same fixture.  Every comparison is exact."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import ref_cand_cases as RC
import ref_ext_cases as XC
import ref_ext_ref as X
import ref_xext_cases as XX

pytestmark = pytest.mark.gpu
FIELDS = ("ok", "qb", "qe", "qs", "sb", "se", "cols")


def reads_volume(M, ctx, read_list):
    pac, nplane, offs, nb = XC.pack_reads(read_list)
    vol = M.Volume(ctx, pac, offs, nb, 0)
    M.volume_set_nplane(ctx, vol, nplane)
    return vol, pac, nplane, offs


class Side:
    """one reference with its reads on the device, and candidates as one table"""

    def __init__(self, M, ctx, ref_fasta, read_list, cands):
        self.M, self.ctx, self.read_list = M, ctx, read_list
        self.g = RC.RefGenome(ref_fasta)
        self.ref, self.idx = self.g.upload(ctx)
        self.reads, self.pac, self.nplane, self.offs = reads_volume(M, ctx, read_list)
        self.n = len(read_list)
        self.tab, self.cnt, self.slot = XC.tables(cands, self.n)
        self.maxc = self.tab.shape[1]

    def run(self, b=0, e=None):
        e = self.n if e is None else e
        return self.M.ref_xextend(self.ctx, self.ref, self.reads, b, e, self.maxc, self.tab[b:e], self.cnt[b:e])

    def strings(self, rid, row, words):
        return XC.lib_strings(row, words, self.pac, self.nplane, self.offs[rid, 0], self.g.pac)

    def free(self):
        self.idx.free(); self.ref.free(); self.reads.free(); self.g.free()


@pytest.fixture(scope="module")
def dev():
    """the fixture's two sets on the device and one run over each"""
    import mecat_amd.hip as M
    fx = XX.fixture()
    ctx = M.Context(0)
    sides, whole, stats = [], [], []
    for k in (0, 1):
        s = fx["sets"][k]
        sd = Side(M, ctx, s["ref_fasta"], s["read_list"], fx["cands"][fx["set"] == k])
        sides.append(sd)
        whole.append(sd.run())
        stats.append(M.ref_xextend_stats())
    yield dict(M=M, fx=fx, ctx=ctx, sides=sides, whole=whole, stats=stats)
    for sd in sides:
        sd.free()
    ctx.close()


def assert_same_run(a, b, what):
    (ra, oa, wa), (rb, ob, wb) = a, b
    assert np.array_equal(ra, rb), what
    assert np.array_equal(oa, ob) and np.array_equal(wa, wb), what


def check_against_fixture(dev, side, res, offs, words, which, slots):
    """fixture candidates `which` sit in slots `slots` of the run (res, offs, words) on set `side`: every numeric field, the matches and the
    CRCs of the rebuilt strings, and for the stored subset the columns word for word"""
    fx, sd = dev["fx"], dev["sides"][side]
    res = res.reshape(-1)
    stored_at = {int(i): j for j, i in enumerate(fx["stored"])}
    n_ok = n_stored = 0
    for i, s in zip(which, slots):
        i, s = int(i), int(s)
        rid, chain, _, _, score = (int(x) for x in fx["cands"][i])
        r = res[s]
        got = tuple(int(r[k]) for k in FIELDS)
        assert got == tuple(int(x) for x in fx["res"][i][:7]), (i, got, fx["res"][i])
        assert (int(r["chain"]), int(r["vscore"])) == (chain, score)
        w = words[int(offs[s]): int(offs[s + 1])]
        if not r["ok"]:
            assert len(w) == 0
            continue
        assert len(w) == (int(r["cols"]) + 15) // 16
        strs = sd.strings(rid, r, w)
        assert strs is not None and (zlib.crc32(strs[0]), zlib.crc32(strs[1])) == tuple(int(x) for x in fx["crc"][i]), i
        a, b = np.frombuffer(strs[0], dtype=np.uint8), np.frombuffer(strs[1], dtype=np.uint8)
        assert int((a == b).sum()) == int(fx["res"][i][7]), i
        n_ok += 1
        if i in stored_at:
            j = stored_at[i]
            assert np.array_equal(w, fx["stored_words"][fx["stored_offs"][j]: fx["stored_offs"][j + 1]]), i
            n_stored += 1
    return n_ok, n_stored


def test_fixture_candidates_through_the_host_entry_point(dev):
    fx = dev["fx"]
    n_ok = n_stored = 0
    for k in (0, 1):
        res, offs, words = dev["whole"][k]
        sd = dev["sides"][k]
        a, b = check_against_fixture(dev, k, res, offs, words, np.flatnonzero(fx["set"] == k), sd.slot)
        n_ok, n_stored = n_ok + a, n_stored + b
        # empty slots: nothing, zero words; the offsets are the running sum of the ok results' words
        flat = res.reshape(-1)
        empty = np.ones(len(flat), dtype=bool)
        empty[sd.slot] = False
        assert not flat[empty]["ok"].any() and not flat[empty]["cols"].any()
        want = np.concatenate([[0], np.cumsum(np.where(flat["ok"] == 1, (flat["cols"] + 15) // 16, 0))])
        assert np.array_equal(offs.astype(np.int64), want) and len(words) == want[-1]
        assert dev["stats"][k]["slots"] == sd.n * sd.maxc and dev["stats"][k]["slices"] == 1
    assert n_ok == int(fx["res"][:, 0].sum()) and n_stored == len(fx["stored"])
    # ok is the query span, not the columns
    flat = dev["whole"][0][0].reshape(-1)
    assert ((flat["cols"] >= 1000) & (flat["ok"] == 0)).sum() >= 10


def test_wide_blocks_on_the_low_complexity_cases_and_none_on_the_plain_ones(dev):
    """the ring block hands a window that outgrows its 126 cells to the wide block, and the stats count those blocks: on the homopolymer /
    tandem reads, and on none of the plain pairs (the crafted ones: a read that is its stretch of random reference, exact or with every
    fourth base substituted, keeps a window of a few dozen cells).  The recorded lists are not plain in this sense: a false candidate's
    extension drifts through unrelated sequence, where hundreds of cells stay within X of the best score."""
    M, fx, sd = dev["M"], dev["fx"], dev["sides"][1]
    assert dev["stats"][1]["redone"] > 0, dev["stats"]
    src = fx["source"][fx["set"] == 1]
    for which in (XX.SRC_CRAFT, XX.SRC_LOWC):
        tab, cnt, slot = XC.tables(fx["cands"][fx["set"] == 1][src == which], sd.n)
        res, _, _ = M.ref_xextend(sd.ctx, sd.ref, sd.reads, 0, sd.n, tab.shape[1], tab, cnt)
        st = M.ref_xextend_stats()
        assert np.array_equal(res.reshape(-1)[slot], dev["whole"][1][0].reshape(-1)[sd.slot[src == which]])
        if which == XX.SRC_CRAFT:
            assert st["redone"] == 0 and int(res["ok"].sum()) == 8, st
        else:
            assert st["redone"] == dev["stats"][1]["redone"], st


@pytest.mark.parametrize("rnd", [0, 1])
def test_device_lists_behind_the_seeding_stage(dev, rnd):
    """seed (-x 1) -> x-extend with nothing copied back in between: the recorded lists' results, slot for slot"""
    M, ctx, fx, sd = dev["M"], dev["ctx"], dev["fx"], dev["sides"][0]
    n = sd.n
    p = M.ref_seed_params(1, maxc=10, round=rnd)
    d_out, d_cnt = C.c_void_p(), C.c_void_p()
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"test_rxx_out", n * 10 * M.REF_CAND_DTYPE.itemsize, C.byref(d_out)))
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"test_rxx_cnt", n * 4, C.byref(d_cnt)))
    M.ref_seed_reads_dev(ctx, sd.idx, sd.ref, sd.reads, 0, n, p, d_out, d_cnt)
    tot = M.ref_xextend_run_dev(ctx, sd.ref, sd.reads, 0, n, 10, d_out, d_cnt)
    res, offs, words = M.ref_extend_fetch(ctx, n, 10, tot)
    which = np.flatnonzero(fx["source"] == rnd + 1)
    # the recorded lists are in call order: the k-th candidate of a read is its slot k
    rd = fx["cands"][which, 0]
    k = np.zeros(len(which), dtype=np.int64)
    for j in range(1, len(k)):
        k[j] = k[j - 1] + 1 if rd[j] == rd[j - 1] else 0
    n_ok, _ = check_against_fixture(dev, 0, res, offs, words, which, rd.astype(np.int64) * 10 + k)
    assert n_ok == int(fx["res"][which, 0].sum()) >= 100
    cnt = np.zeros(n, dtype=np.int32)
    M._chk(M.lib().mhip_download(ctx.h, cnt.ctypes.data, d_cnt, cnt.nbytes))
    assert int(cnt.sum()) == len(which)


def test_slices_equal_one_call(dev):
    """no state leaks between jobs or launches"""
    sd = dev["sides"][0]
    res, offs, words = dev["whole"][0]
    at = 0
    for b, e in ((0, 7), (7, 131), (131, sd.n)):
        r2, o2, w2 = sd.run(b, e)
        assert np.array_equal(r2, res[b:e]), (b, e)
        assert np.array_equal(o2.astype(np.int64) + at, offs[b * sd.maxc: e * sd.maxc + 1].astype(np.int64)), (b, e)
        assert np.array_equal(w2, words[at: at + len(w2)])
        at += len(w2)
    assert at == len(words)
    r2, o2, w2 = sd.run(5, 5)
    assert len(r2) == 0 and len(w2) == 0 and o2.tolist() == [0]


def test_small_column_budget_equals_the_unforced_run(dev):
    M = dev["M"]
    os.environ["MECAT_REF_COLS_BUDGET"] = "20000"          # words: a few jobs per slice
    try:
        got, st = [], []
        for k in (0, 1):
            got.append(dev["sides"][k].run())
            st.append(M.ref_xextend_stats())
    finally:
        del os.environ["MECAT_REF_COLS_BUDGET"]
    assert st[0]["slices"] >= 20 and st[0]["store_words"] <= 40000, st
    assert st[1]["slices"] >= 2 and st[1]["redone"] == dev["stats"][1]["redone"], st          # (the count runs over the slices)
    for k in (0, 1):
        assert_same_run(got[k], dev["whole"][k], "sliced")
    assert_same_run(dev["sides"][0].run(), dev["whole"][0], "again")
    assert M.ref_xextend_stats()["slices"] == 1


def test_every_block_through_the_wide_block_equals_the_default(dev):
    os.environ["MECAT_XD_WIDE"] = "1"
    try:
        got = [dev["sides"][k].run() for k in (0, 1)]
    finally:
        del os.environ["MECAT_XD_WIDE"]
    for k in (0, 1):
        assert_same_run(got[k], dev["whole"][k], "all wide")
    assert_same_run(dev["sides"][1].run(), dev["whole"][1], "the default again")


def edge_case():
    """a 9 kb reference with an N and reads whose start points put 599 / 600 / 601 / int(599 * 1.2) bases on a side, on the read and on the
    reference, windows of 0 and 1 base and windows cut by either end of the reference, on both strands, at 0 - 12 % error, and the
    every-fourth-base pair -> (reference text, reads as letters, cands [m, 5])"""
    rng = np.random.default_rng(4712)
    G = 9000
    g = RC.genome(G, 98)
    let = RC.letters(g).copy()
    let[4000] = ord("N")
    text = RC.fasta_bytes([b"e1", b"e2"], [let[:5000], let[5000:]], width=60)
    reads, cands = [], []

    def add(r, chain, starts):
        r = RC.letters(r).copy()
        if len(reads) % 3 == 0 and len(r) > 300:
            r[100:160] += 32
            r[200] = ord("N")
        if chain:          # the stored read is the other strand: all of it reversed, upper-case letters complemented
            r = X.strand_letters(r, 1).copy()
        rid = len(reads)
        reads.append(r)
        for qs, rs in starts:          # (read_start on the mapped strand, ref_start)
            if 0 <= qs < len(r) and 0 <= rs < G:
                cands.append((rid, chain, rs + 1, qs, 7))
    sides = (599, 600, 601, 718, 719)
    for chain in (0, 1):
        for err in (0.0, 0.06, 0.12):
            m = lambda a, b: XX.mutated(g[a:b], rng, err)
            # the read side: start points `side` bases from the read's two ends
            add(m(1000, 3600), chain, [(s, 1000 + s) for s in sides] + [(2600 - s, 3600 - s) for s in sides if err == 0.0])
            # the reference side: start points `side` bases from the reference's two ends; windows of 0 and 1 base
            add(m(0, 2500), chain, [(s, s) for s in sides] + [(0, 0), (1, 1), (0, 1), (1, 0), (5, 0), (0, 5), (2, 1)])
            r_len = len(reads[-1])
            add(m(G - 2500, G), chain, [(2500 - s, G - s) for s in sides if err == 0.0] + [(100, G - 1), (100, G - 2)])
            cands.append((len(reads) - 1, chain, G, len(reads[-1]) - 1, 7))          # one base to the right on both
            cands.append((len(reads) - 2, chain, 1, r_len - 1, 7))                   # a window of 0 bases to the left, one query base to the right
            # windows cut by either end of the reference: the read hangs over it
            add(np.concatenate([rng.integers(0, 4, 700).astype(np.uint8), m(0, 2000)]), chain, [(1500, 800), (900, 200)])
            add(np.concatenate([m(G - 2000, G), rng.integers(0, 4, 700).astype(np.uint8)]), chain, [(500, G - 1500), (1200, G - 800)])
        # every fourth base substituted from the start point on, and from 300 bases behind it on
        for p in (0, 300):
            add(XX.every_fourth(g[5200:8200], 1400 + p, 1), chain, [(1400, 6600)])
    return text, reads, np.array(cands, dtype=np.int64)


def test_block_size_edges_and_tiny_windows_equal_the_oracle():
    import mecat_amd.hip as M
    text, read_list, cands = edge_case()
    codes, _ = XC.ref_codes(text)
    want = [XX.xgo(codes, read_list[int(c[0])], int(c[1]), int(c[2]), int(c[3])) for c in cands]
    win = np.array([X.window(len(codes), len(read_list[int(c[0])]), int(c[2]), int(c[3])) for c in cands])
    sides = np.concatenate([win[:, 1], win[:, 2], win[:, 3], np.array([w["qs"] for w in want]) - win[:, 1]])
    for s in (0, 1, 599, 600, 601, 718):
        assert (sides == s).any(), s
    assert sum(w["ok"] for w in want) >= 20
    ctx = M.Context(0)
    sd = Side(M, ctx, text, read_list, cands)
    res, woffs, words = sd.run()
    flat = res.reshape(-1)
    one_column_left = 0
    for i, (w, s) in enumerate(zip(want, sd.slot)):
        r = flat[int(s)]
        assert tuple(int(r[k]) for k in FIELDS) == tuple(w[k] for k in FIELDS), (i, cands[i], r, w)
        if not w["ok"]:
            continue
        strs = sd.strings(int(cands[i][0]), r, words[int(woffs[s]): int(woffs[s + 1])])
        assert strs is not None, (i, cands[i])          # (the query and target bases in the strings equal the spans)
        a, b = np.frombuffer(strs[0], dtype=np.uint8), np.frombuffer(strs[1], dtype=np.uint8)
        assert int((a == b).sum()) == w["matches"], (i, cands[i])
        assert int((a != 45).sum()) == w["qe"] - w["qb"] and int((b != 45).sum()) == w["se"] - w["sb"]
        one_column_left += int(cands[i][3] - w["qb"] + cands[i][2] - 1 - w["sb"] == 0 and win[i][1] >= 1 and win[i][2] >= 1)
    assert one_column_left >= 1          # a left half the drop rule empties
    sd.free(); ctx.close()


def test_refusals_leave_the_context_working(dev):
    M, ctx, sd = dev["M"], dev["ctx"], dev["sides"][0]
    n, maxc = sd.n, sd.maxc
    # the PacBio entry point still refuses the technology, and names the call that takes it
    with pytest.raises(M.MhipError, match="nanopore"):
        M.ref_extend(ctx, sd.ref, sd.reads, 0, n, maxc, sd.tab, sd.cnt, tech=1)
    rng = np.random.default_rng(5)
    long_reads, _, _, _ = reads_volume(M, ctx, [RC.letters(rng.integers(0, 4, 99999)), RC.letters(rng.integers(0, 4, 100000))])
    tab = np.zeros((2, 1), dtype=M.REF_CAND_DTYPE)
    tab["loc1"], tab["loc2"] = 10, 10
    res, _, _ = M.ref_xextend(ctx, sd.ref, long_reads, 0, 1, 1, tab[:1], np.ones(1, dtype=np.int32))          # 99 999 letters: extended
    assert res[0, 0]["qs"] == 99999
    with pytest.raises(M.MhipError, match="100000"):
        M.ref_xextend(ctx, sd.ref, long_reads, 0, 2, 1, tab, np.ones(2, dtype=np.int32))
    long_reads.free()
    G = sd.g.num_bases
    r0 = int(np.flatnonzero(sd.cnt)[0])
    for field, value in (("loc1", 0), ("loc1", G + 1), ("loc2", -1), ("loc2", len(sd.read_list[r0]))):
        bad = sd.tab.copy()
        bad[r0, 0][field] = value
        with pytest.raises(M.MhipError, match="outside"):
            M.ref_xextend(ctx, sd.ref, sd.reads, 0, n, maxc, bad, sd.cnt)
    bad_cnt = sd.cnt.copy()
    bad_cnt[r0] = maxc + 1
    with pytest.raises(M.MhipError, match="outside"):
        M.ref_xextend(ctx, sd.ref, sd.reads, 0, n, maxc, sd.tab, bad_cnt)
    assert_same_run(sd.run(), dev["whole"][0], "after the refusals")


def test_a_pacbio_run_afterwards_still_equals_its_fixture(dev):
    """the two aligners share jobs, buffers and the fetch: a DiffAligner run behind the X-drop ones gives what ref_ext.npz records"""
    M, ctx, sd = dev["M"], dev["ctx"], dev["sides"][0]
    pb = XC.fixture()
    tab, cnt, slot = XC.tables(pb["cands"], sd.n)
    res, offs, words = M.ref_extend(ctx, sd.ref, sd.reads, 0, sd.n, tab.shape[1], tab, cnt)
    flat = res.reshape(-1)
    n_ok = 0
    for i, s in enumerate(slot):
        r = flat[int(s)]
        assert tuple(int(r[k]) for k in XC.RES_FIELDS) == tuple(int(x) for x in pb["res"][i]), i
        if r["ok"]:
            strs = sd.strings(int(pb["cands"][i][0]), r, words[int(offs[s]): int(offs[s + 1])])
            assert strs is not None and (zlib.crc32(strs[0]), zlib.crc32(strs[1])) == tuple(int(x) for x in pb["crc"][i]), i
            n_ok += 1
    assert n_ok == int(pb["res"][:, 0].sum())
    assert_same_run(sd.run(), dev["whole"][0], "x-drop again")
