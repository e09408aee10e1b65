"""mhip_xalign_candidates (xd_extend_w: xd_block_ring.h, xd_block_wide.h, XTail) at the window, traceback and trim edges that
tests/xd_edge_cases.py constructs and tests/test_xd_edge_cases_cpu.py proves to be there: results against orc_xdrop_go, the four
arrangements against each other, and the work counters against the walker over the oracle's row trace.  Every comparison is exact.

What the counters count (xalign.hip, xd_extend_w): slot 3 is one per block that was STARTED in the ring or, all-wide, in the wide block; a
block redone in place is not counted again (slot 33 counts those).  Slots 32 and 4 add a block's rows and cells per run of a block, so a
redone block adds the rows of its abandoned ring run as well: they equal the trace's sums where no block is redone, and always under
MECAT_XD_WIDE=1.  Rows are rows entered, cells the windows at the rows' entries summed: the trace's definitions."""
import os

import numpy as np
import pytest

import helpers as H
import xd_edge_cases as E

pytestmark = pytest.mark.gpu
NAMES = "ABCDE"


@pytest.fixture(scope="module")
def hip():
    import mecat_amd.hip as M
    return M


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vols(hip, ctx):
    """name -> (family, its reads as a volume, its jobs), made on first use"""
    made = {}

    def get(name):
        if name not in made:
            f = E.ladder_below() if name == "A-below" else E.everything() if name == "all" else E.family(name)
            lens = np.array([len(s) for s in f.seqs], dtype=np.int32)
            ov = H.orc_pack(np.concatenate(f.seqs).astype(np.uint8), lens)
            offs, pac = H.vol_arrays(ov)
            made[name] = (f, hip.Volume(ctx, pac, offs, ov.contents.num_bases, 0), np.array(f.jobs, dtype=hip.JOB_DTYPE))
        return made[name]
    yield get
    for _, v, _ in made.values():
        v.free()


def run(hip, ctx, vol, jobs, min_aln=1, **env):
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return hip.align_candidates(ctx, vol, vol, jobs, min_aln, tech=1).copy()
    finally:
        for k in env:
            os.environ.pop(k)


def fields(r):
    return tuple(int(r[k]) for k in E.FIELDS)


def assert_equals_the_oracle(f, out, min_aln):
    bad = []
    for i, (q, t, qs, ts, lab) in enumerate(f.pairs):
        want = E.go(q, qs, t, ts, min_aln)
        if fields(out[i]) != want:
            bad.append((i, lab, f.jobs[i], fields(out[i]), want))
    assert not bad, "%d of %d jobs differ from orc_xdrop_go: %s" % (len(bad), len(f.jobs), bad[:4])


@pytest.mark.parametrize("name", NAMES)
def test_results_equal_the_oracle(hip, ctx, vols, name):
    """min_align_size 1, so that ok hides no short result; family D (block geometry) also at 500"""
    f, vol, jobs = vols(name)
    out = run(hip, ctx, vol, jobs, 1)
    assert_equals_the_oracle(f, out, 1)
    # the block counts: what the walker chained, per job (both halves)
    want_blocks = [len(w["left"]) + len(w["right"]) for w in f.walks()]
    assert out["blocks"].tolist() == want_blocks
    if name == "D":
        assert_equals_the_oracle(f, run(hip, ctx, vol, jobs, 500), 500)


@pytest.mark.parametrize("name", NAMES)
def test_arrangements_give_the_same_bytes(hip, ctx, vols, name, capfd):
    """in place (the default), hand-over, all-wide and candidate order: byte-equal results.  Family E under hand-over: the units the ring
    launch lists for the second launch are the units the walker says have a block that outgrows the ring, and they resume in their
    second or third block, in the left half as well as in the right one (test_family_e_overflow_behind_the_first_block)."""
    f, vol, jobs = vols(name)
    base = run(hip, ctx, vol, jobs, 1)
    capfd.readouterr()
    handed = run(hip, ctx, vol, jobs, 1, MECAT_XD_HANDOVER=1, MECAT_TRACE=1)
    err = capfd.readouterr().err
    assert handed.tobytes() == base.tobytes(), np.flatnonzero(handed != base)[:5]
    # (the text is xd_launch_ring's fprintf under MECAT_TRACE in xalign.hip: "X-drop: %u of %d units need the wide-window path")
    nwide = int(err.split("X-drop: ")[1].split(" of ")[0])
    assert nwide == f.totals()["wide_units"], err
    for env in (dict(MECAT_XD_WIDE=1), dict(MECAT_XD_ORDER=0), dict(MECAT_XD_ORDER=0, MECAT_XD_HANDOVER=1)):
        got = run(hip, ctx, vol, jobs, 1, **env)
        assert got.tobytes() == base.tobytes(), (env, np.flatnonzero(got != base)[:5])


def test_longest_first_order_really_sorts_and_changes_nothing(hip, ctx, vols):
    """xd_order_jobs sorts only where there are more jobs than resident waves: with one ring wave per CU (MECAT_XW_WAVES=1) the jobs of
    all families together (more than 4 000) are more, so the default sorts them and MECAT_XD_ORDER=0 does not.  Few waves also means every wave runs
    many units of every kind one behind the other: no state leaks from a unit into the next."""
    f, vol, jobs = vols("all")
    assert len(jobs) > 4000
    base = run(hip, ctx, vol, jobs, 1)
    assert_equals_the_oracle(f, base, 1)
    ctx.set_profiling(True)          # (launches are listed by name only while profiling is on)
    try:
        ctx.reset_stats()
        sorted_run = run(hip, ctx, vol, jobs, 1, MECAT_XW_WAVES=1)
        assert "xo_place" in ctx.kernel_stats(), ctx.kernel_stats().keys()          # (the sort's last launch)
        ctx.reset_stats()
        unsorted = run(hip, ctx, vol, jobs, 1, MECAT_XW_WAVES=1, MECAT_XD_ORDER=0)
        assert "xo_place" not in ctx.kernel_stats() and "xd_extend_w" in ctx.kernel_stats()
    finally:
        ctx.set_profiling(False)
    handed = run(hip, ctx, vol, jobs, 1, MECAT_XW_WAVES=1, MECAT_XD_ORDER=0, MECAT_XD_HANDOVER=1)
    for got in (sorted_run, unsorted, handed):
        assert got.tobytes() == base.tobytes(), np.flatnonzero(got != base)[:5]


def counters(ctx):
    return dict(blocks=ctx.debug_counter(3), cells=ctx.debug_counter(4), rows=ctx.debug_counter(32), redone=ctx.debug_counter(33))


@pytest.mark.parametrize("name", NAMES)
def test_counters_equal_the_trace(hip, ctx, vols, name):
    f, vol, jobs = vols(name)
    tot = f.totals()
    ctx.reset_stats()
    run(hip, ctx, vol, jobs, 1)
    got = counters(ctx)
    print("family %s, default: %s; the walker: %s" % (name, got, tot))
    assert got["redone"] == tot["redone"]          # exactly the blocks whose window passes 126 cells
    assert got["blocks"] == tot["blocks"]          # (a redone block is one block)
    if tot["redone"] == 0:
        assert (got["rows"], got["cells"]) == (tot["rows"], tot["cells"])
    ctx.reset_stats()
    run(hip, ctx, vol, jobs, 1, MECAT_XD_WIDE=1)
    got = counters(ctx)
    print("family %s, all wide: %s" % (name, got))
    assert got == dict(blocks=tot["blocks"], cells=tot["cells"], rows=tot["rows"], redone=0)


def test_ladder_below_the_threshold_redoes_nothing_and_counts_the_trace(hip, ctx, vols):
    """family A up to 126 cells: none of these blocks leaves the ring (the full family's count is exactly the blocks above: the test
    above), and the ring block's own rows and cells equal the trace's"""
    f, vol, jobs = vols("A-below")
    tot = f.totals()
    assert tot["redone"] == 0
    ctx.reset_stats()
    out = run(hip, ctx, vol, jobs, 1)
    assert_equals_the_oracle(f, out, 1)
    assert counters(ctx) == dict(blocks=tot["blocks"], cells=tot["cells"], rows=tot["rows"], redone=0)
