"""mecat2ref on the device, stage 1: the reference file's volume and index (mecat_amd/host/ref_genome.cpp +
mhip_index_build) and mhip_ref_seed_reads (mecat_amd/csrc/ref_seed.hip) against the candidate lists the UNMODIFIED mecat2ref recorded
(tests/golden/ref_cand.npz, tests/golden/make_golden_ref_cand.py) and, beyond the fixture, against the plain restatement
tests/ref_cand_ref.py, which tests/test_ref_cand_cpu.py pins to the same fixture."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_cand_cases as RC
import ref_cand_ref as R

pytestmark = pytest.mark.gpu


def reads_volume(M, ctx, read_list):
    pac, nplane, offs, nb = RC.pack_reads(read_list)
    vol = M.Volume(ctx, pac, offs, nb, 0)
    M.volume_set_nplane(ctx, vol, nplane)
    return vol


@pytest.fixture(scope="module")
def dev():
    """the fixture's reference and reads on the device"""
    import mecat_amd.hip as M
    fx = RC.fixture()
    ctx = M.Context(0)
    g = RC.RefGenome(fx["ref_fasta"].tobytes())
    ref, idx = g.upload(ctx)
    reads = reads_volume(M, ctx, fx["read_list"])
    yield dict(M=M, fx=fx, ctx=ctx, g=g, ref=ref, idx=idx, reads=reads, n=len(fx["read_list"]))
    idx.free(); ref.free(); reads.free(); g.free(); ctx.close()


def lists_of(out, cnt):
    """(cands [n, maxc], counts) -> per read int64[count, 10] in RC.FIELDS order"""
    assert (cnt >= 0).all() and (cnt <= out.shape[1]).all()
    return [np.stack([out[i, :c][f].astype(np.int64) for f in RC.FIELDS], axis=1) if c else np.zeros((0, 10), dtype=np.int64) for i, c in enumerate(cnt)]


def assert_lists_equal(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and (a == b).all(), (what, i, a, b)


def test_index_of_the_reference_equals_creat_ref_index(dev):
    fx = dev["fx"]
    let, _ = R.read_reference(fx["ref_fasta"].tobytes())
    want = R.Index(let)
    counts, offsets = dev["idx"].download()
    wc = np.zeros(1 << 26, dtype=np.int32)
    wc[want.keys] = want.cnt
    assert np.array_equal(counts, wc)
    # ids ascending == the order of offsets[]; positions 0-based here, ascending inside a bucket
    wpos = np.concatenate([want.pos[f: f + c] for f, c in zip(want.first, want.cnt)]) - 1
    assert np.array_equal(offsets, wpos.astype(np.int32))
    ids = [int("".join(str(int(x)) for x in p), 4) for p in fx["plants"]]
    assert len(ids) == 5 and all(counts[i] == 0 for i in ids)
    assert all(int((R.kmer_ids(let) == i).sum()) > 128 for i in ids)


@pytest.mark.parametrize("rnd", [0, 1])
@pytest.mark.parametrize("tech,maxc", RC.RUNS)
def test_candidates_equal_the_recorded_lists(dev, tech, maxc, rnd):
    M, ctx, n = dev["M"], dev["ctx"], dev["n"]
    want = RC.recorded(dev["fx"], tech, maxc, rnd + 1)
    p = M.ref_seed_params(tech, maxc=maxc, round=rnd)
    out, cnt = M.ref_seed_reads(ctx, dev["idx"], dev["ref"], dev["reads"], 0, n, p)
    assert_lists_equal(lists_of(out, cnt), want, "host")
    # the same through the entry point that leaves the lists on the device
    d_out, d_cnt = C.c_void_p(), C.c_void_p()
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"test_ref_out", out.nbytes, C.byref(d_out)))
    M._chk(M.lib().mhip_ctx_buffer(ctx.h, b"test_ref_cnt", cnt.nbytes, C.byref(d_cnt)))
    M.ref_seed_reads_dev(ctx, dev["idx"], dev["ref"], dev["reads"], 0, n, p, d_out, d_cnt)
    out2, cnt2 = np.zeros_like(out), np.zeros_like(cnt)
    M._chk(M.lib().mhip_download(ctx.h, cnt2.ctypes.data, d_cnt, cnt2.nbytes))
    M._chk(M.lib().mhip_download(ctx.h, out2.ctypes.data, d_out, out2.nbytes))
    assert_lists_equal(lists_of(out2, cnt2), want, "dev")


def test_slices_equal_one_call(dev):
    """no state leaks between reads or launches"""
    M, ctx, n = dev["M"], dev["ctx"], dev["n"]
    for rnd in (0, 1):
        p = M.ref_seed_params(0, round=rnd)
        whole = lists_of(*M.ref_seed_reads(ctx, dev["idx"], dev["ref"], dev["reads"], 0, n, p))
        parts = []
        for b, e in ((0, 7), (7, 131), (131, n)):
            parts += lists_of(*M.ref_seed_reads(ctx, dev["idx"], dev["ref"], dev["reads"], b, e, p))
        assert_lists_equal(parts, whole, "slices")
        assert_lists_equal(whole, RC.recorded(dev["fx"], 0, 10, rnd + 1), "whole")
    out, cnt = M.ref_seed_reads(ctx, dev["idx"], dev["ref"], dev["reads"], 5, 5, p)
    assert len(cnt) == 0


def test_small_record_pool_goes_through_the_second_launch(dev):
    M, ctx, n = dev["M"], dev["ctx"], dev["n"]
    os.environ["MECAT_REF_POOL"] = "8"
    try:
        for rnd in (0, 1):
            p = M.ref_seed_params(0, round=rnd)
            got = lists_of(*M.ref_seed_reads(ctx, dev["idx"], dev["ref"], dev["reads"], 0, n, p))
            st = M.ref_seed_stats()
            assert st["reads"] == n and st["pool"] == 8 and st["redone"] >= 20, st
            assert_lists_equal(got, RC.recorded(dev["fx"], 0, 10, rnd + 1), "small pool")
    finally:
        del os.environ["MECAT_REF_POOL"]
    M.ref_seed_reads(ctx, dev["idx"], dev["ref"], dev["reads"], 0, n, p)
    assert M.ref_seed_stats()["redone"] == 0


def test_long_read_and_bad_arguments_are_refused(dev):
    M, ctx = dev["M"], dev["ctx"]
    rng = np.random.default_rng(5)
    reads = reads_volume(M, ctx, [RC.letters(rng.integers(0, 4, 99999)), RC.letters(rng.integers(0, 4, 100000))])
    p = M.ref_seed_params(0)
    out, cnt = M.ref_seed_reads(ctx, dev["idx"], dev["ref"], reads, 0, 1, p)          # 99 999 letters: mapped (a random read: nothing)
    assert cnt[0] == 0
    with pytest.raises(M.MhipError, match="100000"):
        M.ref_seed_reads(ctx, dev["idx"], dev["ref"], reads, 0, 2, p)
    with pytest.raises(M.MhipError, match="list length"):
        M.ref_seed_reads(ctx, dev["idx"], dev["ref"], reads, 0, 1, M.ref_seed_params(0, maxc=101))
    with pytest.raises(M.MhipError, match="round"):
        M.ref_seed_reads(ctx, dev["idx"], dev["ref"], reads, 0, 1, M.ref_seed_params(0, round=2))
    with pytest.raises(M.MhipError, match="read range"):
        M.ref_seed_reads(ctx, dev["idx"], dev["ref"], reads, 0, 3, p)
    reads.free()


def fresh_case():
    """a 40 kb reference in two records (an N run, single other letters, a 1.5 kb repeat) and 300 reads of 10 to 3 000 letters at 0 - 15 %
    error from both strands, some with lower-case and N letters, some random"""
    rng = np.random.default_rng(77)
    g = RC.genome(40000, 4242)
    g[30000:31500] = g[5000:6500]
    let = RC.letters(g).copy()
    let[12000:12045] = ord("N")
    let[[700, 25000, 39990]] = [ord("N"), ord("Y"), ord("n")]
    let[100:400] += 32
    text = RC.fasta_bytes([b"one", b"two x"], [let[:23000], let[23000:]], width=60)
    reads = []
    for i in range(300):
        kind = i % 10
        L = int(rng.integers(10, 3001)) if kind else int(rng.integers(10, 40))
        if kind == 9:
            r = RC.letters(rng.integers(0, 4, L)).copy()
        else:
            r = RC.letters(RC.one_read(g, i, L, float(rng.choice([0.0, 0.05, 0.10, 0.15])), 99)).copy()
        if kind == 8 and len(r) > 100:
            a = int(rng.integers(0, len(r) - 50))
            r[a: a + 40] += 32
            r[int(rng.integers(0, len(r)))] = ord("N")
        reads.append(r)
    return text, reads


@pytest.mark.parametrize("rnd,cutoff,maxc", [(0, 0.25, 10), (0, 0.1, 2), (1, 0.1, 4)])
def test_fresh_reads_equal_the_restatement(rnd, cutoff, maxc):
    import mecat_amd.hip as M
    text, read_list = fresh_case()
    let, _ = R.read_reference(text)
    want_idx = R.Index(let)
    want = [R.candidates(want_idx, r, rnd, cutoff, maxc) for r in read_list]
    assert sum(1 for w in want if len(w)) >= 100 and (maxc == 10 or sum(1 for w in want if len(w) == maxc) >= 1)
    ctx = M.Context(0)
    g = RC.RefGenome(text)
    ref, idx = g.upload(ctx)
    reads = reads_volume(M, ctx, read_list)
    p = M.ref_seed_params(0, maxc=maxc, round=rnd, ddfs_cutoff=cutoff)
    got = lists_of(*M.ref_seed_reads(ctx, idx, ref, reads, 0, len(read_list), p))
    assert_lists_equal(got, want, "fresh")
    idx.free(); ref.free(); reads.free(); g.free(); ctx.close()

