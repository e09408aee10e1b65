"""mecat2ref on the device, stage 2: mhip_ref_extend_run / _run_dev / _fetch (mecat_amd/csrc/ref_extend.hip) against what
the UNMODIFIED extend_candidate recorded (tests/golden/ref_ext.npz, tests/golden/make_golden_ref_ext.py) and, beyond the fixture, against
the plain restatement tests/ref_ext_ref.py, which tests/test_ref_ext_cpu.py pins to the same fixture."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import ref_cand_cases as RC
import ref_ext_cases as XC
import ref_ext_ref as X

pytestmark = pytest.mark.gpu


def reads_volume(M, ctx, read_list):
    pac, nplane, offs, nb = XC.pack_reads(read_list)
    vol = M.Volume(ctx, pac, offs, nb, 0)
    M.volume_set_nplane(ctx, vol, nplane)
    return vol, pac, nplane, offs


@pytest.fixture(scope="module")
def dev():
    """the fixture's reference and reads on the device, its candidates as one table, and one run over all of them"""
    import mecat_amd.hip as M
    fx = XC.fixture()
    ctx = M.Context(0)
    g = RC.RefGenome(fx["ref_fasta"])
    ref, idx = g.upload(ctx)
    reads, pac, nplane, offs = reads_volume(M, ctx, fx["read_list"])
    n = len(fx["read_list"])
    tab, cnt, slot = XC.tables(fx["cands"], n)
    d = dict(M=M, fx=fx, ctx=ctx, g=g, ref=ref, idx=idx, reads=reads, n=n, pac=pac, nplane=nplane, offs=offs, tab=tab, cnt=cnt, slot=slot, maxc=tab.shape[1])
    d["whole"] = M.ref_extend(ctx, ref, reads, 0, n, d["maxc"], tab, cnt)
    yield d
    idx.free(); ref.free(); reads.free(); g.free(); ctx.close()


def assert_same_run(a, b, what):
    (ra, oa, wa), (rb, ob, wb) = a, b
    assert np.array_equal(ra, rb), what
    assert np.array_equal(oa, ob) and np.array_equal(wa, wb), what


def check_against_fixture(dev, res, offs, words, which, slots):
    """fixture candidates `which` sit in slots `slots` of the run (res, offs, words): every numeric field, the CRCs of the rebuilt strings,
    and for the stored subset the columns word for word"""
    fx = dev["fx"]
    res = res.reshape(-1)
    stored_at = {int(i): j for j, i in enumerate(fx["stored"])}
    n_ok = n_stored = 0
    for i, s in zip(which, slots):
        i, s = int(i), int(s)
        rid, chain, _, _, score = (int(x) for x in fx["cands"][i])
        r = res[s]
        got = tuple(int(r[k]) for k in XC.RES_FIELDS)
        assert got == tuple(int(x) for x in fx["res"][i]), (i, got, fx["res"][i])
        assert (int(r["chain"]), int(r["vscore"])) == (chain, score)
        w = words[int(offs[s]): int(offs[s + 1])]
        if not r["ok"]:
            assert len(w) == 0
            continue
        assert len(w) == (int(r["cols"]) + 15) // 16
        strs = XC.lib_strings(r, w, dev["pac"], dev["nplane"], dev["offs"][rid, 0], dev["g"].pac)
        assert strs is not None and (zlib.crc32(strs[0]), zlib.crc32(strs[1])) == tuple(int(x) for x in fx["crc"][i]), i
        n_ok += 1
        if i in stored_at:
            j = stored_at[i]
            assert np.array_equal(w, fx["stored_words"][fx["stored_offs"][j]: fx["stored_offs"][j + 1]]), i
            n_stored += 1
    return n_ok, n_stored


def test_fixture_candidates_through_the_host_entry_point(dev):
    fx = dev["fx"]
    res, offs, words = dev["whole"]
    n_ok, n_stored = check_against_fixture(dev, res, offs, words, np.arange(len(fx["cands"])), dev["slot"])
    assert n_ok == int(fx["res"][:, 0].sum()) and n_stored == len(fx["stored"])
    # empty slots: nothing, zero words; the offsets are the running sum of the ok results' words
    flat = res.reshape(-1)
    empty = np.ones(len(flat), dtype=bool)
    empty[dev["slot"]] = False
    assert not flat[empty]["ok"].any() and not flat[empty]["cols"].any()
    want = np.concatenate([[0], np.cumsum(np.where(flat["ok"] == 1, (flat["cols"] + 15) // 16, 0))])
    assert np.array_equal(offs.astype(np.int64), want) and len(words) == want[-1]
    st = dev["M"].ref_extend_stats()
    assert st["slots"] == dev["n"] * dev["maxc"] and st["slices"] == 1


@pytest.mark.parametrize("rnd", [0, 1])
def test_device_lists_behind_the_seeding_stage(dev, rnd):
    """seed -> extend with nothing copied back in between: the recorded lists' results, slot for slot"""
    M, ctx, n, fx = dev["M"], dev["ctx"], dev["n"], dev["fx"]
    p = M.ref_seed_params(0, maxc=10, round=rnd)
    d_out, d_cnt = C.c_void_p(), C.c_void_p()
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"test_rx_out", n * 10 * M.REF_CAND_DTYPE.itemsize, C.byref(d_out)))
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"test_rx_cnt", n * 4, C.byref(d_cnt)))
    M.ref_seed_reads_dev(ctx, dev["idx"], dev["ref"], dev["reads"], 0, n, p, d_out, d_cnt)
    tot = M.ref_extend_run_dev(ctx, dev["ref"], dev["reads"], 0, n, 10, d_out, d_cnt)
    res, offs, words = M.ref_extend_fetch(ctx, n, 10, tot)
    which = np.flatnonzero(fx["source"] == rnd + 1)
    # the recorded lists are in call order: the k-th candidate of a read is its slot k
    rd = fx["cands"][which, 0]
    k = np.zeros(len(which), dtype=np.int64)
    for j in range(1, len(k)):
        k[j] = k[j - 1] + 1 if rd[j] == rd[j - 1] else 0
    n_ok, _ = check_against_fixture(dev, res, offs, words, which, rd.astype(np.int64) * 10 + k)
    assert n_ok == int(fx["res"][which, 0].sum()) >= 100
    cnt = np.zeros(n, dtype=np.int32)
    M._chk(M.lib().mhip_download(ctx.h, cnt.ctypes.data, d_cnt, cnt.nbytes))
    assert int(cnt.sum()) == len(which)


def test_stage_one_lists_with_the_new_packing_equal_the_recorded_lists(dev):
    M, ctx, n = dev["M"], dev["ctx"], dev["n"]
    base = RC.fixture()
    for rnd in (0, 1):
        out, cnt = M.ref_seed_reads(ctx, dev["idx"], dev["ref"], dev["reads"], 0, n, M.ref_seed_params(0, maxc=10, round=rnd))
        want = RC.recorded(base, 0, 10, rnd + 1)
        assert [int(c) for c in cnt] == [len(w) for w in want]
        for i, w in enumerate(want):
            got = np.stack([out[i, :len(w)][f].astype(np.int64) for f in RC.FIELDS], axis=1) if len(w) else np.zeros((0, 10), dtype=np.int64)
            assert (got == w).all(), (rnd, i)


def test_slices_equal_one_call(dev):
    """no state leaks between jobs or launches"""
    M, ctx, n, maxc = dev["M"], dev["ctx"], dev["n"], dev["maxc"]
    res, offs, words = dev["whole"]
    at = 0
    for b, e in ((0, 7), (7, 131), (131, n)):
        r2, o2, w2 = M.ref_extend(ctx, dev["ref"], dev["reads"], b, e, maxc, dev["tab"][b:e], dev["cnt"][b:e])
        assert np.array_equal(r2, res[b:e]), (b, e)
        assert np.array_equal(o2.astype(np.int64) + at, offs[b * maxc: e * maxc + 1].astype(np.int64)), (b, e)
        assert np.array_equal(w2, words[at: at + len(w2)])
        at += len(w2)
    assert at == len(words)
    r2, o2, w2 = M.ref_extend(ctx, dev["ref"], dev["reads"], 5, 5, maxc, dev["tab"][5:5], dev["cnt"][5:5])
    assert len(r2) == 0 and len(w2) == 0 and o2.tolist() == [0]


def test_small_column_budget_equals_the_unforced_run(dev):
    M, ctx, n, maxc = dev["M"], dev["ctx"], dev["n"], dev["maxc"]
    os.environ["MECAT_REF_COLS_BUDGET"] = "20000"          # words: a few jobs per slice
    try:
        got = M.ref_extend(ctx, dev["ref"], dev["reads"], 0, n, maxc, dev["tab"], dev["cnt"])
        st = M.ref_extend_stats()
    finally:
        del os.environ["MECAT_REF_COLS_BUDGET"]
    assert st["slices"] >= 20 and st["store_words"] <= 40000, st
    assert_same_run(got, dev["whole"], "sliced")
    got = M.ref_extend(ctx, dev["ref"], dev["reads"], 0, n, maxc, dev["tab"], dev["cnt"])
    assert M.ref_extend_stats()["slices"] == 1
    assert_same_run(got, dev["whole"], "again")


def mutated(g, rng, err):
    """a forward copy of g with substitutions, insertions and deletions at rate err -> codes"""
    out = []
    for b in g:
        u = rng.random()
        if u < err / 3:
            continue
        if u < 2 * err / 3:
            out.append(int(rng.integers(0, 4)))
        out.append(int(b) if u >= err else int((b + 1 + rng.integers(0, 3)) % 4))
    return np.array(out, dtype=np.uint8)


def edge_case():
    """a 9 kb reference with an N and reads whose start points put 599 / 600 / 601 / int(599 * 1.2) bases on a side, on the read and on the
    reference, and windows of 0 and 1 base, on both strands, at 0 - 12 % error -> (reference text, reads as letters, cands [m, 5])"""
    rng = np.random.default_rng(4711)
    G = 9000
    g = RC.genome(G, 99)
    let = RC.letters(g).copy()
    let[4000] = ord("N")
    text = RC.fasta_bytes([b"e1", b"e2"], [let[:5000], let[5000:]], width=60)
    reads, cands = [], []

    def add(a, b, err, chain, starts):
        r = RC.letters(mutated(g[a:b], rng, err)).copy()
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
            # the read side: start points `side` bases from the read's two ends
            add(1000, 3600, err, chain, [(s, 1000 + s) for s in sides] + [(2600 - s, 3600 - s) for s in sides if err == 0.0])
            # the reference side: start points `side` bases from the reference's two ends
            add(0, 2500, err, chain, [(s, s) for s in sides] + [(0, 0), (1, 1), (0, 1), (1, 0), (5, 0), (0, 5)])
            r_len = len(reads[-1])
            add(G - 2500, G, err, chain, [(2500 - s, G - s) for s in sides if err == 0.0] + [(100, G - 1), (100, G - 2)])
            cands.append((len(reads) - 1, chain, G, len(reads[-1]) - 1, 7))          # one base to the right on both
            cands.append((len(reads) - 2, chain, 1, r_len - 1, 7))                   # a window of 0 bases to the left, one query base to the right
    return text, reads, np.array(cands, dtype=np.int64)


def test_block_size_edges_and_tiny_windows_equal_the_restatement():
    import mecat_amd.hip as M
    text, read_list, cands = edge_case()
    codes, _ = XC.ref_codes(text)
    want = [X.extend(codes, read_list[int(c[0])], int(c[1]), int(c[2]), int(c[3])) for c in cands]
    win = np.array([X.window(len(codes), len(read_list[int(c[0])]), int(c[2]), int(c[3])) for c in cands])
    sides = np.concatenate([win[:, 1], win[:, 2], win[:, 3], np.array([w["qs"] for w in want]) - win[:, 1]])
    for s in (0, 1, 599, 600, 601, 718):
        assert (sides == s).any(), s
    assert sum(w["ok"] for w in want) >= 20 and sum(1 for w in want if w["ok"] and (w["left"]["sized_last"] or w["right"]["sized_last"])) >= 5
    ctx = M.Context(0)
    g = RC.RefGenome(text)
    ref, idx = g.upload(ctx)
    reads, pac, nplane, offs = reads_volume(M, ctx, read_list)
    tab, cnt, slot = XC.tables(cands, len(read_list))
    res, woffs, words = M.ref_extend(ctx, ref, reads, 0, len(read_list), tab.shape[1], tab, cnt)
    flat = res.reshape(-1)
    for i, (w, s) in enumerate(zip(want, slot)):
        r = flat[int(s)]
        assert tuple(int(r[k]) for k in XC.RES_FIELDS) == tuple(w[k] for k in XC.RES_FIELDS), (i, cands[i], r, {k: w[k] for k in XC.RES_FIELDS})
        if w["ok"]:
            assert np.array_equal(words[int(woffs[s]): int(woffs[s + 1])], X.columns_of(w["qmap"], w["smap"])), (i, cands[i])
    idx.free(); ref.free(); reads.free(); g.free(); ctx.close()


def test_refusals_leave_the_context_working(dev):
    M, ctx, n, maxc = dev["M"], dev["ctx"], dev["n"], dev["maxc"]
    with pytest.raises(M.MhipError, match="nanopore"):
        M.ref_extend(ctx, dev["ref"], dev["reads"], 0, n, maxc, dev["tab"], dev["cnt"], tech=1)
    rng = np.random.default_rng(5)
    long_reads, _, _, _ = reads_volume(M, ctx, [RC.letters(rng.integers(0, 4, 99999)), RC.letters(rng.integers(0, 4, 100000))])
    tab = np.zeros((2, 1), dtype=M.REF_CAND_DTYPE)
    tab["loc1"], tab["loc2"] = 10, 10
    res, _, _ = M.ref_extend(ctx, dev["ref"], long_reads, 0, 1, 1, tab[:1], np.ones(1, dtype=np.int32))          # 99 999 letters: extended
    assert res[0, 0]["qs"] == 99999
    with pytest.raises(M.MhipError, match="100000"):
        M.ref_extend(ctx, dev["ref"], long_reads, 0, 2, 1, tab, np.ones(2, dtype=np.int32))
    long_reads.free()
    G = dev["g"].num_bases
    r0 = int(np.flatnonzero(dev["cnt"])[0])
    for field, value in (("loc1", 0), ("loc1", G + 1), ("loc2", -1), ("loc2", len(dev["fx"]["read_list"][r0]))):
        bad = dev["tab"].copy()
        bad[r0, 0][field] = value
        with pytest.raises(M.MhipError, match="outside"):
            M.ref_extend(ctx, dev["ref"], dev["reads"], 0, n, maxc, bad, dev["cnt"])
    bad_cnt = dev["cnt"].copy()
    bad_cnt[r0] = maxc + 1
    with pytest.raises(M.MhipError, match="outside"):
        M.ref_extend(ctx, dev["ref"], dev["reads"], 0, n, maxc, dev["tab"], bad_cnt)
    assert_same_run(M.ref_extend(ctx, dev["ref"], dev["reads"], 0, n, maxc, dev["tab"], dev["cnt"]), dev["whole"], "after the refusals")
