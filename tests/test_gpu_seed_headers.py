"""seed_strand fetches the bucket headers of its strands itself (seed_probe runs only for strands left to the kernel chain) and is
persistent: one workgroup per CU, strands taken from a cursor, the next strand's headers requested while the current one is built.
Every case: candidate lists == the oracle's == a second run with MECAT_SEED_FUSED_PROBE=0 (seed_probe first, seed_strand copies its
headers from the km_* arrays), and the lookup / bucket-hit counters of both runs are equal."""
import json
import os
from contextlib import contextmanager

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

SEGCAP = 6144          # FS_SEGCAP (seed_strand.hip): k-mers of a strand whose headers fit the LDS of seed_strand


@pytest.fixture(scope="module")
def hip():
    import mecat_amd.hip as M
    return M


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    c.set_profiling(True)          # (kernel_stats: which kernels ran, how often)
    yield c
    c.close()


@contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def kmers(L):
    return 0 if L < 13 else (int(L) - 13) // 10 + 1


class Vol:
    def __init__(self, hip, ctx, codes, lens, start=0):
        self.lens = np.asarray(lens, dtype=np.int32)
        self.ov = H.orc_pack(codes, self.lens, start)
        self.offs, pac = H.vol_arrays(self.ov)
        self.nb = self.ov.contents.num_bases
        self.gv = hip.Volume(ctx, pac, self.offs, self.nb, start)

    def free(self):
        self.gv.free()


def run(hip, ctx, gi, ref, reads, p, a=0, b=None):
    """-> (lists, counts, dict(lookups, hits, took, left, kernels)) of one call"""
    b = len(reads.lens) if b is None else b
    ctx.reset_stats()
    got, cnt = hip.seed_reads(ctx, gi, ref.gv, reads.gv, a, b, p)
    c = ctx.counters()
    ks = ctx.kernel_stats()
    st = dict(lookups=c["lookups"], hits=c["hits"], took=ctx.debug_counter(13), left=ctx.debug_counter(14), walked=ctx.debug_counter(15),
              kernels={k: v[0] for k, v in ks.items()})
    return got, cnt, st


def same_lists(got, cnt, got2, cnt2):
    assert np.array_equal(cnt, cnt2)
    for r in range(len(cnt)):
        assert np.array_equal(got[r][: cnt[r]], got2[r][: cnt[r]]), r


def vs_oracle(got, cnt, want):
    bad = [r for r, w in enumerate(want) if not (cnt[r] == len(w) and all(np.array_equal(got[r][: cnt[r]][f], w[f]) for f in H.CAND_DTYPE.names))]
    assert not bad, "%d reads differ from the oracle, first %d" % (len(bad), bad[0])


def both_ways(hip, ctx, gi, ref, reads, p, want, a=0, b=None, same_split=True):
    """the call with the headers fetched by seed_strand and with seed_probe in front: lists == oracle, equal counters -> stats of the first"""
    got, cnt, st = run(hip, ctx, gi, ref, reads, p, a, b)
    with env(MECAT_SEED_FUSED_PROBE=0):
        got2, cnt2, st2 = run(hip, ctx, gi, ref, reads, p, a, b)
    vs_oracle(got, cnt, want)
    same_lists(got, cnt, got2, cnt2)
    nk = 2 * sum(kmers(L) for L in reads.lens[a:b])
    print("lookups %d / %d (expected %d), hits %d / %d, walked %d / %d, strands taken %d / %d, left %d / %d; kernels %s" % (
        st["lookups"], st2["lookups"], nk, st["hits"], st2["hits"], st["walked"], st2["walked"], st["took"], st2["took"], st["left"], st2["left"],
        st["kernels"]))
    assert st["lookups"] == st2["lookups"] == nk
    assert st["hits"] == st2["hits"] and st["walked"] == st2["walked"]
    if same_split:      # (not when the strands race for too little room: which of them find it differs from run to run)
        assert (st["took"], st["left"]) == (st2["took"], st2["left"])
    assert st2["kernels"].get("seed_probe", 0) == st2["kernels"]["seed_strand"] >= 1      # the knob restores the order probe, strand
    if st["left"] == 0:
        assert "seed_probe" not in st["kernels"], st["kernels"]                            # no strand for the chain: no probe at all
    else:
        assert st["kernels"].get("seed_probe", 0) >= 1
    return got, cnt, st


def mutate(rng, r, err):
    r = r.copy()
    m = rng.random(len(r)) < err
    r[m] = (r[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
    return r


def test_lookup_count_edges(hip, ctx):
    """K = 0, 1, around one and two records per thread of the 1 024-thread workgroup (1 023 .. 1 025, 2 047 .. 2 049), ~3 000 (a third
    record per thread: fetched at the top of the iteration), and one read above FS_SEGCAP k-mers.  The fallen-back strands are told by
    their number only: two more with the long read in the call than without it, as many strands built by seed_strand either way.
    Whether a strand's headers were requested ahead or fetched at the top of its iteration depends on which workgroup drew it and
    when (76 strands: hardly a workgroup takes a second one), so this test does not claim each K on the prefetched path; wrong headers
    on either path show in the comparison with the oracle.  test_more_strands_than_workgroups is the one that loops."""
    rng = np.random.default_rng(17)
    G0 = rng.integers(0, 4, size=90000).astype(np.uint8)
    ks = [0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 3003, 1, 1024, 2048, 2049, 1025]
    lens = [7] + [13 + 10 * (k - 1) for k in ks[1:]]
    lens += [int(x) for x in rng.integers(2500, 6000, size=24)]
    klong = SEGCAP + 57
    lens.append(13 + 10 * (klong - 1))                  # 62 013 bases: the last read
    reads = []
    for i, L in enumerate(lens):
        st = int(rng.integers(0, len(G0) - L + 1))
        r = mutate(rng, G0[st:st + L], 0.10)
        if i % 3 == 1:
            r = (3 - r)[::-1].copy()
        reads.append(r.astype(np.uint8))
    lens = np.array(lens, dtype=np.int32)
    assert [kmers(L) for L in lens[:len(ks)]] == ks and kmers(lens[-1]) == klong > SEGCAP
    v = Vol(hip, ctx, np.concatenate(reads), lens)
    gi = hip.Index(ctx, v.gv)
    p = hip.default_params(0)
    want = H.orc_seed_all(v.ov, v.ov, H.orc().orc_index_build(v.ov), H.orc_params(tech=0))
    n = len(lens)
    # without the long read: nothing is left to the chain, and the strands that keep hits are there
    _, _, st = both_ways(hip, ctx, gi, v, v, p, want[:n - 1], 0, n - 1)
    nfwd = int((lens[:n - 1] >= 2500).sum())             # (a forward strand meets its own copy: it keeps hits)
    assert st["left"] == 0 and st["took"] >= nfwd, (st, nfwd)
    # with it: its two strands, nothing else
    got, cnt, st2 = both_ways(hip, ctx, gi, v, v, p, want)
    assert st2["left"] == 2 and st2["took"] == st["took"], (st, st2)
    assert int(cnt.sum()) > 50 and cnt[-1] > 0
    gi.free()
    v.free()


@pytest.fixture(scope="module")
def many(hip, ctx):
    """401 reads of 3 kb: 802 strands, three rounds and a part of a fourth for the workgroups of a 256-CU device, both directions
    (test_more_strands_than_workgroups checks the premise against the device's CU count)"""
    codes, lens = H.synth_reads(401, 3000, 0.15, 60000, 23)
    v = Vol(hip, ctx, codes, lens)
    gi = hip.Index(ctx, v.gv)
    oidx = H.orc().orc_index_build(v.ov)
    want = H.orc_seed_all(v.ov, v.ov, oidx, H.orc_params(tech=0))
    yield dict(v=v, gi=gi, want=want)
    gi.free()
    v.free()


def test_more_strands_than_workgroups(hip, ctx, many):
    v = many["v"]
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count      # seed_strand launches one workgroup per CU
    assert len(v.lens) % 2 == 1 and len(v.lens) >= 1.5 * cus and (2 * len(v.lens)) % cus != 0, cus
    got, cnt, st = both_ways(hip, ctx, many["gi"], v, v, hip.default_params(0), many["want"])
    assert st["left"] == 0 and st["took"] >= len(v.lens), st
    assert st["kernels"]["seed_strand"] == 1
    assert int((got["chain"][np.arange(got.shape[1])[None, :] < cnt[:, None]] == 0).sum()) > 0       # candidates of both directions
    assert int((got["chain"][np.arange(got.shape[1])[None, :] < cnt[:, None]] == 1).sum()) > 0


def test_headers_from_cut_records(hip, ctx, many):
    """the diagonal cell with the cuts on (what test_more_strands_than_workgroups runs): the premise, reads whose bucket lengths come from a
    byte below 7 of the cut record and reads at byte 7 (seed_probe's rule on index.hip's cut step), and that the cuts shorten the walk"""
    v = many["v"]
    segs = (int(v.nb) + 1999) // 2000
    step = ((segs + 7) // 8) * 2000
    t = (v.offs[:, 0].astype(np.int64) + v.offs[:, 1] + 1 + 5 * 2000 + step - 1) // step
    assert int((t <= 7).sum()) > 50 and int((t > 7).sum()) > 10, (step, t.min(), t.max())
    _, _, st = both_ways(hip, ctx, many["gi"], v, v, hip.default_params(0), many["want"])
    assert 0 < st["walked"] < st["hits"], st


def test_headers_from_starts_on_the_diagonal(hip, ctx, many):
    """MECAT_SEED_CUTS=0: every bucket to its end, headers from starts[]"""
    v = many["v"]
    with env(MECAT_SEED_CUTS=0):
        _, _, st = both_ways(hip, ctx, many["gi"], v, v, hip.default_params(0), many["want"])
    assert st["walked"] == 0 and st["left"] == 0 and st["took"] >= len(v.lens), st


def test_headers_from_starts_off_the_diagonal(hip, ctx):
    """an off-diagonal two-volume cell: no cut records"""
    codes, lens = H.synth_reads(300, 3000, 0.15, 40000, 21)
    cut = 170
    nb = int(lens[:cut].sum())
    v0 = Vol(hip, ctx, codes[:nb], lens[:cut], 0)
    v1 = Vol(hip, ctx, codes[nb:], lens[cut:], cut)
    gi = hip.Index(ctx, v0.gv)
    want = H.orc_seed_all(v0.ov, v1.ov, H.orc().orc_index_build(v0.ov), H.orc_params(tech=0))
    got, cnt, st = both_ways(hip, ctx, gi, v0, v1, hip.default_params(0), want)
    assert st["walked"] == 0 and st["left"] == 0 and st["took"] >= len(v1.lens), st
    assert int(cnt.sum()) > 50
    for x in (gi, v0, v1):
        x.free()


def test_fallback_gets_its_probe(hip, ctx, many):
    """the shared output arrays too small for all strands: some are built by seed_strand, the others by the kernel chain, which reads the
    km_* arrays — seed_probe runs behind seed_strand then, once, and tallies nothing a second time (both_ways compares the counters)"""
    v = many["v"]
    with env(MECAT_SEED_FUSED_ROOM=20000):
        _, _, st = both_ways(hip, ctx, many["gi"], v, v, hip.default_params(0), many["want"], same_split=False)
    assert st["took"] > 0 and st["left"] > 0, st
    assert st["kernels"]["seed_probe"] == 1 and st["kernels"]["seed_build"] == 1, st


def test_several_launches(hip, ctx):
    """MECAT_SEED_BATCH_HITS at its floor: three launches of seed_strand, each with a cleared cursor and no header request beyond its last
    strand: the lists of the one-launch call"""
    codes, lens = H.synth_reads(700, 8000, 0.15, 500000, 29)
    v = Vol(hip, ctx, codes, lens)
    gi = hip.Index(ctx, v.gv)
    p = hip.default_params(0)
    one, cnt1, st1 = run(hip, ctx, gi, v, v, p)
    assert st1["kernels"]["seed_strand"] == 1 and "seed_probe" not in st1["kernels"]
    with env(MECAT_SEED_BATCH_HITS=1e6):
        got, cnt, st = run(hip, ctx, gi, v, v, p)
        with env(MECAT_SEED_FUSED_PROBE=0):
            got2, cnt2, st2 = run(hip, ctx, gi, v, v, p)
    print(st1, st, st2)
    assert st["kernels"]["seed_strand"] >= 3 and st2["kernels"]["seed_strand"] == st["kernels"]["seed_strand"] == st2["kernels"]["seed_probe"]
    vs_oracle(one, cnt1, H.orc_seed_all(v.ov, v.ov, H.orc().orc_index_build(v.ov), H.orc_params(tech=0)))
    same_lists(one, cnt1, got, cnt)
    same_lists(one, cnt1, got2, cnt2)
    for k in ("lookups", "hits", "walked", "took", "left"):
        assert st1[k] == st[k] == st2[k], k
    assert st["lookups"] == 2 * sum(kmers(L) for L in lens) and int(cnt.sum()) > 1000
    gi.free()
    v.free()


def sort_passes(num_bases):
    """seed_batch's rule: the segment ids of the reference volume (num_bases / 2000 is the highest) in passes of up to 11 bits"""
    nbits = max(1, int(num_bases // 2000).bit_length())
    return (nbits + 10) // 11


def test_kernels_launched_per_path(hip, ctx):
    """Which seeding kernels one seed_reads call launches, and how often, for every way through seed_batch, on the golden sets tiny
    (PacBio gate 2 * min_kmer_match >= 6: relevance filter and strand pipeline on) and tiny_ont (nanopore gate in [4, 6): the wide filter,
    no strand pipeline).  One batch each (the sets are far below the batch budget): seed_cand runs once.
      pipeline on, every strand taken          seed_strand, seed_cand; no seed_probe, nothing of the chain
      pipeline on, strands left (ROOM=64)      seed_strand, then seed_probe once and the chain behind it
      MECAT_SEED_FUSED=0 / MECAT_SEED_FILTER=0 no seed_strand: seed_probe first, the chain with seed_filter (FILTER=0 turns the pipeline off too)
      nanopore                                 the same with seed_filter_wide in the place of seed_filter
    The chain = filter, seed_scan, seed_emit, one seed_sort_pass per 11 bits of a segment id, seed_build."""
    G = json.load(open(os.path.join(H.GOLDEN, "golden.json")))

    def load(name):
        g = G["sets"][name]["gen"]
        codes, lens = H.synth_reads(g["nreads"], g["L"], g["err"], g["genome"], g["seed"], g["ont"])
        v = Vol(hip, ctx, codes, lens)
        return v, hip.Index(ctx, v.gv), hip.default_params(g["ont"])

    def chain(filter_kernel, passes):
        return {"seed_probe": 1, filter_kernel: 1, "seed_scan": 1, "seed_emit": 1, "seed_sort_pass": passes, "seed_build": 1, "seed_cand": 1}

    def launched(v, gi, p, **knobs):
        with env(**knobs):
            _, cnt, st = run(hip, ctx, gi, v, v, p)
        assert int(cnt.sum()) > 100, knobs       # every path has hits to emit, sort and build
        print(knobs, st)
        return {k: n for k, n in st["kernels"].items() if k.startswith("seed_")}, st

    v, gi, p = load("tiny")
    passes = sort_passes(v.nb)
    assert 2 * p.min_kmer_match >= 6 and passes == 1
    got, st = launched(v, gi, p)
    assert st["left"] == 0 and st["took"] > 0
    assert got == {"seed_strand": 1, "seed_cand": 1}
    got, st = launched(v, gi, p, MECAT_SEED_FUSED=0)
    assert got == chain("seed_filter", passes) and (st["took"], st["left"]) == (0, 0)
    got, st = launched(v, gi, p, MECAT_SEED_FILTER=0)
    assert got == chain("seed_filter", passes) and (st["took"], st["left"]) == (0, 0)
    got, st = launched(v, gi, p, MECAT_SEED_FUSED_ROOM=64)
    assert st["left"] > 0                        # (a forward strand meets its own copy: hundreds of kept hits, 64 places)
    assert got == dict(chain("seed_filter", passes), seed_strand=1)
    gi.free()
    v.free()

    v, gi, p = load("tiny_ont")
    passes = sort_passes(v.nb)
    assert 4 <= 2 * p.min_kmer_match < 6 and passes == 1
    got, st = launched(v, gi, p)
    assert got == chain("seed_filter_wide", passes) and (st["took"], st["left"]) == (0, 0)
    assert got["seed_sort_pass"] == sort_passes(v.nb)
    gi.free()
    v.free()
    # (two passes: 2^11 segments and more, a volume of 4.1 Mbase — test_gpu_fullsize.py runs those)
    assert [sort_passes(n) for n in (2000 * 2047 + 1999, 2000 * 2048, 2000 * (1 << 21))] == [1, 2, 2]
