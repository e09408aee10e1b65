"""seed_cand keeps a copy of 64 gated segments' records and scores in its lanes, takes the neighbours of both sweeps 32 a side per
round with the lists of eight segments in flight, and asks for the subject lookup's block entry ahead of the vote threshold.
Every case: candidate lists == the oracle's, every field.  The sets are the smallest that reach each path, and each asserts from the
oracle's lists that it still does: lists that fill and shift (maxc = 5), sweeps over 8 to 20 segments on both sides, sweeps of more
than 32 and more than 64 segments a side (second and third round), segments that overflow SM (lists from ent_fin), tables from
seed_strand, from the kernel chain and from both in one launch, several batches, and a cell whose reference is not the reads."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import mecat_amd.hip as M
    return M


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    c.set_profiling(True)          # (kernel_stats: how often seed_cand ran)
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


class Vol:
    def __init__(self, hip, ctx, codes, lens, start=0):
        self.lens = np.asarray(lens, dtype=np.int32)
        self.ov = H.orc_pack(codes, self.lens, start)
        self.offs, pac = H.vol_arrays(self.ov)
        self.gv = hip.Volume(ctx, pac, self.offs, self.ov.contents.num_bases, start)

    def free(self):
        self.gv.free()


class Cell:
    """one set as its own reference: the device's volume and index, and the oracle's lists for every maxc asked for (computed once)"""

    def __init__(self, hip, ctx, codes, lens):
        self.hip, self.ctx = hip, ctx
        self.v = Vol(hip, ctx, codes, lens)
        self.gi = hip.Index(ctx, self.v.gv)
        self.oidx = H.orc().orc_index_build(self.v.ov)
        self._want = {}

    def want(self, maxc=100):
        if maxc not in self._want:
            self._want[maxc] = H.orc_seed_all(self.v.ov, self.v.ov, self.oidx, H.orc_params(tech=0, maxc=maxc))
        return self._want[maxc]

    def run(self, maxc=100, **knobs):
        """-> stats of one seed_reads call under the knobs, its lists compared with the oracle's"""
        with env(**knobs):
            st = seed(self.hip, self.ctx, self.gi, self.v, self.v, self.hip.default_params(0, maxc=maxc), self.want(maxc))
        print(knobs, st)
        return st

    def free(self):
        self.gi.free()
        self.v.free()


def seed(hip, ctx, gi, ref, reads, p, want):
    ctx.reset_stats()
    got, cnt = hip.seed_reads(ctx, gi, ref.gv, reads.gv, 0, len(reads.lens), p)
    bad = [r for r, w in enumerate(want) if not (cnt[r] == len(w) and all(np.array_equal(got[r][: cnt[r]][f], w[f]) for f in H.CAND_DTYPE.names))]
    assert not bad, "%d reads differ from the oracle, first %d" % (len(bad), bad[0])
    ks = ctx.kernel_stats()
    return dict(took=ctx.debug_counter(13), left=ctx.debug_counter(14), kernels={k: v[0] for k, v in ks.items() if k.startswith("seed_")})


def cat(want):
    return np.concatenate(want)


@pytest.fixture(scope="module")
def set_a(hip, ctx):
    c = Cell(hip, ctx, *H.synth_reads(300, 6000, 0.15, 60000, 11))
    w, w5 = c.want(100), c.want(5)
    assert len(cat(w)) == 3973 and max(len(x) for x in w) == 40
    assert (cat(w)["chain"] == 0).any() and (cat(w)["chain"] == 1).any()
    assert sum(len(x) == 5 for x in w5) == 242                       # lists that fill: the insertion shifts and drops
    yield c
    c.free()


@pytest.fixture(scope="module")
def set_b(hip, ctx):
    c = Cell(hip, ctx, *H.synth_reads(60, 40000, 0.15, 300000, 12))
    a = cat(c.want())
    assert len(a) == 433
    assert int((a["num2"] >= 16000).sum()) == 256 and int((a["num2"] >= 24000).sum()) == 167 and int((a["num1"] >= 16000).sum()) == 22
    yield c
    c.free()


# the knobs of seed_batch a set is run under, and what the call must have done for the case to be the one it says it is
KNOBS = {
    "default": (dict(), lambda st: st["took"] > 0 and st["kernels"]["seed_cand"] == 1),
    "chain_tables": (dict(MECAT_SEED_FUSED=0), lambda st: st["took"] == 0 and "seed_strand" not in st["kernels"] and st["kernels"]["seed_build"] == 1),
    "both_tables": (dict(MECAT_SEED_FUSED_ROOM=20000), lambda st: st["took"] > 0 and st["left"] > 0 and st["kernels"]["seed_cand"] == 1),
    "no_predrop": (dict(MECAT_SEED_PREDROP=0), lambda st: st["kernels"]["seed_cand"] == 1),
    # (the knob's floor: sets A and B stay below it and make one batch; test_several_batches has the set that makes three)
    "batch_floor": (dict(MECAT_SEED_BATCH_HITS=1e6), lambda st: st["kernels"]["seed_cand"] >= 1),
}


@pytest.mark.parametrize("knobs", sorted(KNOBS))
@pytest.mark.parametrize("maxc", [100, 5])
def test_set_a(set_a, maxc, knobs):
    kw, premise = KNOBS[knobs]
    st = set_a.run(maxc, **kw)
    assert premise(st), st


@pytest.mark.parametrize("knobs", sorted(KNOBS))
def test_set_b_long_sweeps(set_b, knobs):
    kw, premise = KNOBS[knobs]
    st = set_b.run(100, **kw)
    assert premise(st), st


def test_several_batches(hip, ctx):
    """700 reads of 8 kb with MECAT_SEED_BATCH_HITS at its floor: three launches of seed_cand, each on its own batch's reads"""
    c = Cell(hip, ctx, *H.synth_reads(700, 8000, 0.15, 500000, 29))
    assert len(cat(c.want())) > 1000
    st = c.run(MECAT_SEED_BATCH_HITS=1e6)
    assert st["kernels"]["seed_cand"] >= 3, st
    c.free()


def test_reference_is_not_the_reads(hip, ctx):
    """an off-diagonal cell of two volumes: subject ids from the reference's block table and start id, no self hit"""
    codes, lens = H.synth_reads(300, 6000, 0.15, 60000, 11)
    cut = 170
    nb = int(lens[:cut].sum())
    v0, v1 = Vol(hip, ctx, codes[:nb], lens[:cut], 0), Vol(hip, ctx, codes[nb:], lens[cut:], cut)
    gi = hip.Index(ctx, v0.gv)
    want = H.orc_seed_all(v0.ov, v1.ov, H.orc().orc_index_build(v0.ov), H.orc_params(tech=0))
    assert len(cat(want)) > 1000 and int(cat(want)["readno"].max()) < cut
    st = seed(hip, ctx, gi, v0, v1, hip.default_params(0), want)
    assert st["kernels"]["seed_cand"] == 1
    for x in (gi, v0, v1):
        x.free()


def test_overflowed_segments(hip, ctx):
    """a repeat-rich set: segments with more than SM hits, their final lists replayed into ent_fin (the oracle's 41st-seed rule meets
    hits of other reads and throws entries out), lists that reach maxc"""
    codes, lens, _ = H.synth_reads_rep(200, 5000, 0.08, 80000, 601, 0, 10, 80, 25)
    c = Cell(hip, ctx, codes, lens)
    H.orc_stats_reset()
    w = c.want()
    s = H.orc_stats()
    assert s["non_self"] > 10000 and s["dropped"] > 10000 and sum(len(x) == 100 for x in w) > 100, s
    c.run()
    c.run(MECAT_SEED_FUSED=0)
    c.free()


def test_more_than_64_neighbours_on_a_side(hip, ctx):
    """six reads of 168 kb on a genome of 220 kb: sweeps of more than 32 segments (a second round of neighbours) on both sides and of more
    than 64 (a third) on both sides"""
    c = Cell(hip, ctx, *H.synth_reads(6, 160000, 0.15, 220000, 13))
    a = cat(c.want())
    assert int((a["num1"] > 64000).sum()) >= 6 and int((a["num2"] > 64000).sum()) >= 9
    assert int((a["num1"] > 128000).sum()) >= 1 and int((a["num2"] > 128000).sum()) >= 9
    c.run()
    c.free()
