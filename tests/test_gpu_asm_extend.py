"""SURVEY.md §8f row N3, the extension of mecat2canu's overlappers at function level: mhip_asm_extend, mhip_asm_extend_run and
mhip_asm_extend_fetch (mecat_amd/csrc/asm_extend.hip: ae_word_offsets, ae_pack; cns_extend.hip: cns_extend<true>) against tests/golden/asm_ext.npz — the
aligned strings the UNMODIFIED pairwise_mapping of mecat2asmpw.c left for every candidate (oracle/ref_harness_asmpw_ext.c,
tests/golden/make_golden_asm_ext.py), turned into the header's five counts per direction and its 2-bit columns.  Read sets: the golden
2 % set with either block indexed, corrected reads at 4 / 5 / 6 % and at 10 / 12 % error (only the last two make `align`'s limit of 0.10
of the two blocks' bases bind: it counts O(ND) differences), reads with N and with IUPAC codes (second plane), and hand-built pairs: the
bases available to a direction stepping one base at a time across the 600-base edge of the block loop and across 1 100, seeds within
13 bases of a read end, one direction of more than 40 000 columns.  Every comparison is exact.  mecat2trimpw.c's loop is the same text
as mecat2asmpw.c's (no constant differs), so the one fixture stands for both tools.
Columns are kept in full for every third job and for the hand-built sets, as a SHA-256 per direction for all of them."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

sys.path.insert(0, H.GOLDEN)

# symbols of the characters that are not A, C, G, T, as mecat_amd/asmpw/asmpw_main.cpp hands them out: (code in the volume, value in the
# second plane); any one-to-one assignment compares the same
_CODE = np.zeros(256, dtype=np.uint8)
_PLANE = np.zeros(256, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i
for _ch, (_c, _p) in zip(b"NRYKMSWBDHVX", [(0, 3), (1, 3), (2, 3), (3, 3), (0, 1), (1, 1), (2, 1), (3, 1), (0, 2), (1, 2), (2, 2), (3, 2)]):
    _CODE[_ch], _PLANE[_ch] = _c, _p


class Fixture:
    def __init__(self):
        self.z = np.load(os.path.join(H.GOLDEN, "asm_ext.npz"))
        self.meta = json.loads(self.z["meta"].tobytes().decode())
        self.jobs = self.z["jobs"]
        self.dirs = self.z["dirs"]
        self.sha = self.z["sha256"]
        offs, words = self.z["full_offs"], self.z["full_words"]
        self.full = {int(k): words[offs[i]: offs[i + 1]] for i, k in enumerate(self.z["full_dirs"])}
        self.specs = {s["name"]: s for s in self.meta["sets"]}

    def set_jobs(self, name):
        import mecat_amd.hip as M
        a, b = self.meta["ranges"][name]
        return np.ascontiguousarray(self.jobs[a:b]).view(M.ASM_JOB_DTYPE).reshape(-1), a


_fx = None


def fixture():
    global _fx
    if _fx is None:
        _fx = Fixture()
    return _fx


def make_volume(ctx, texts, start_id):
    import mecat_amd.hip as M
    from mecat_amd import workload as W
    arr = np.frombuffer(b"".join(texts), dtype=np.uint8)
    lens = np.array([len(t) for t in texts], dtype=np.int32)
    assert (_PLANE[arr] != 0).sum() == (~np.isin(arr, list(b"ACGT"))).sum(), "a character without a symbol"
    pac, offs, nb = W.pack_volume(_CODE[arr], lens)
    vol = M.Volume(ctx, pac, offs, nb, start_id)
    plane = _PLANE[arr]
    if plane.any():
        idx = (np.repeat(np.asarray(offs)[:, 0].astype(np.int64), lens) + np.arange(len(arr)) - np.repeat(np.cumsum(lens) - lens, lens))
        npac = np.zeros(len(pac), dtype=np.uint8)
        at = plane != 0
        np.bitwise_or.at(npac, idx[at] >> 2, (plane[at] << ((~idx[at] & 3) << 1)).astype(np.uint8))
        M.volume_set_nplane(ctx, vol, npac)
    return vol


def open_set(ctx, name):
    """-> (block volume, mapped reads volume, jobs, index of the first job in the fixture, dir_cols_cap as the tools size it)"""
    import make_golden_asm_ext as G
    fx = fixture()
    block, first_no, queries = G.set_reads(fx.specs[name], fx.z)
    bvol = make_volume(ctx, block, first_no)
    qvol = make_volume(ctx, [q for _, q in queries], queries[0][0])
    jobs, first = fx.set_jobs(name)
    maxlen = max(max(len(t) for t in block), max(len(q) for _, q in queries))
    return bvol, qvol, jobs, first, ((maxlen * 2 + 64 + 15) // 16) * 16


def words_of(ops_row, cols):
    """the ceil(cols / 16) words of one direction as the device wrote them: the bits behind column `cols` in the last word are compared
    too — the header defines them as zero, the dense consumers and the fixture's padding count on it"""
    return np.array(ops_row[: (cols + 15) // 16], dtype="<u4")


def check_against_fixture(name, jobs, first, dirs, ops_of):
    """dirs [2 n, 6] and ops_of(k) -> the words of direction k, against the fixture's records of jobs first .. first + n"""
    fx = fixture()
    n = len(jobs)
    want = fx.dirs[2 * first: 2 * (first + n)]
    bad = np.nonzero((dirs[:, :5] != want).any(axis=1))[0]
    assert not len(bad), "%s: job %s direction %d: counts %s, the reference has %s (%d directions differ)" % (
        name, jobs[bad[0] // 2], bad[0] % 2, dirs[bad[0]].tolist(), want[bad[0]].tolist(), len(bad))
    assert not dirs[:, 5].any()
    for k in range(2 * n):
        cols = int(dirs[k, 0])
        w = words_of(ops_of(k), cols)
        full = fx.full.get(2 * first + k)
        if full is not None and not np.array_equal(w, full):
            a = ((w[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).reshape(-1)[:cols]
            b = ((full[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).reshape(-1)[:cols]
            c = int(np.nonzero(a != b)[0][0])
            raise AssertionError("%s: job %s direction %d: column %d is %d, the reference has %d" % (name, jobs[k // 2], k % 2, c, a[c], b[c]))
        assert hashlib.sha256(w.tobytes()).digest() == fx.sha[2 * first + k].tobytes(), "%s: job %s direction %d: columns differ from the reference's (hash only)" % (
            name, jobs[k // 2], k % 2)


ALL_SETS = ["golden_S1", "golden_S2", "err4", "err5", "err6", "err10", "err12", "with_n", "iupac", "ladder_r", "ladder_l", "edges", "long"]


def test_the_parametrised_tests_name_every_set_of_the_fixture():
    assert ALL_SETS == [s["name"] for s in fixture().meta["sets"]]


@pytest.mark.parametrize("name", ALL_SETS)
def test_extension_equals_the_reference_column_by_column(name):
    """mhip_asm_extend on every job of the set: the five counts of every direction and every column [0, cols) as the unmodified tool
    strung them together; then the dense form of the same batch (mhip_asm_extend_run / _fetch): the same dirs, word_offs the running sum
    of ceil(cols / 16), total_words their sum, every direction's words the fixed-stride call's."""
    import mecat_amd.hip as M
    ctx = M.Context(0)
    bvol, qvol, jobs, first, cap = open_set(ctx, name)
    dirs, ops = M.asm_extend(ctx, bvol, qvol, jobs, cap)
    check_against_fixture(name, jobs, first, dirs, lambda k: ops[k])
    total = M.asm_extend_run(ctx, bvol, qvol, jobs, cap)
    ddirs, offs, dense = M.asm_extend_fetch(ctx, len(jobs), total)
    check_dense(dirs, ops, ddirs, offs, dense, total)
    bvol.free(); qvol.free(); ctx.close()


def check_dense(dirs, ops, ddirs, offs, dense, total):
    nw = (dirs[:, 0].astype(np.int64) + 15) // 16
    assert np.array_equal(ddirs, dirs)
    assert offs[0] == 0 and np.array_equal(np.diff(offs.astype(np.int64)), nw)
    assert total == int(nw.sum()) == int(offs[-1]) == len(dense)
    for k in range(len(dirs)):
        a = dense[int(offs[k]): int(offs[k + 1])]
        assert np.array_equal(a, ops[k, : nw[k]]), "direction %d: dense words differ from the fixed-stride call's" % k


@pytest.mark.parametrize("njobs", [1, 512, 1024, 1300])
def test_dense_hand_over_across_the_scan_steps(njobs):
    """ae_word_offsets scans 1 024 directions a step and carries the sum: batches of 2 directions, of exactly 1 024 and 2 048 (ending on
    a step) and of 2 600 (two carries, a partial last step), made by repeating the golden set's jobs — against the fixed-stride call on the
    same batch, which is itself held to the fixture."""
    import mecat_amd.hip as M
    ctx = M.Context(0)
    bvol, qvol, jobs, first, cap = open_set(ctx, "golden_S1")
    batch = jobs[np.arange(njobs) % len(jobs)]
    dirs, ops = M.asm_extend(ctx, bvol, qvol, batch, cap)
    m = min(njobs, len(jobs))
    check_against_fixture("golden_S1", batch[:m], first, dirs[: 2 * m], lambda k: ops[k])
    total = M.asm_extend_run(ctx, bvol, qvol, batch, cap)
    ddirs, offs, dense = M.asm_extend_fetch(ctx, njobs, total)
    assert 2 * njobs in (2, 1024, 2048, 2600)
    check_dense(dirs, ops, ddirs, offs, dense, total)
    bvol.free(); qvol.free(); ctx.close()


@pytest.mark.parametrize("name", ALL_SETS)
def test_results_do_not_depend_on_the_batch(name):
    """every job of the set in one call, in a permuted order, and all of them again in calls of 1, of 3 and of 257 jobs on the same
    context: the same counts and words per job (the work cursor, the per-wave scratch a wave reuses from job to job, the N planes staged
    after a job without them)."""
    import mecat_amd.hip as M
    ctx = M.Context(0)
    bvol, qvol, jobs, first, cap = open_set(ctx, name)
    n = len(jobs)
    dirs, ops = M.asm_extend(ctx, bvol, qvol, jobs, cap)
    check_against_fixture(name, jobs, first, dirs, lambda k: ops[k])
    perm = np.random.default_rng(5).permutation(n)
    pd, po = M.asm_extend(ctx, bvol, qvol, jobs[perm], cap)
    sel = np.stack([2 * perm, 2 * perm + 1], axis=1).reshape(-1)
    assert np.array_equal(pd, dirs[sel]) and np.array_equal(po, ops[sel])
    for size in (1, 3, 257):
        for a in range(0, n, size):
            b = min(n, a + size)
            sd, so = M.asm_extend(ctx, bvol, qvol, jobs[a:b], cap)
            assert np.array_equal(sd, dirs[2 * a: 2 * b]) and np.array_equal(so, ops[2 * a: 2 * b]), (size, a)
    bvol.free(); qvol.free(); ctx.close()


@pytest.mark.parametrize("name", ["err4", "err5", "err6", "err10", "err12"])
def test_jobs_built_from_the_device_candidates(name):
    """index, mhip_asm_seed_reads and asm_jobs_from_candidates on the set, then the extension: every job of the fixture is among the
    device's jobs, and gives the fixture's counts and columns."""
    import mecat_amd.hip as M
    fx = fixture()
    ctx = M.Context(0)
    bvol, qvol, jobs, first, cap = open_set(ctx, name)
    idx = M.Index(ctx, bvol, max_bucket=256)
    cands, cnt = M.asm_seed_reads(ctx, idx, bvol, qvol, 0, qvol.num_reads)
    djobs = M.asm_jobs_from_candidates(cands, cnt)
    assert len(djobs) == int(cnt.sum()) > 100
    at = {j.tobytes(): i for i, j in enumerate(djobs)}
    pick = [at.get(j.tobytes()) for j in jobs]
    assert None not in pick, "%d of the fixture's %d jobs are not among the device's candidates" % (pick.count(None), len(jobs))
    dirs, ops = M.asm_extend(ctx, bvol, qvol, djobs, cap)
    sel = np.stack([2 * np.array(pick), 2 * np.array(pick) + 1], axis=1).reshape(-1)
    check_against_fixture(name, jobs, first, dirs[sel], lambda k: ops[sel[k]])
    assert fx.meta["ranges"][name][1] - fx.meta["ranges"][name][0] == len(jobs)
    idx.free(); bvol.free(); qvol.free(); ctx.close()


def test_refusals_leave_the_context_usable():
    """error returns only: a dir_cols_cap that is not a multiple of 16, a cap smaller than a direction needs, a start point outside its
    read, and a _fetch for another number of jobs than the last _run — each with its message, each followed by a good call."""
    import mecat_amd.hip as M
    ctx = M.Context(0)
    bvol, qvol, jobs, first, cap = open_set(ctx, "golden_S2")
    jobs = jobs[:64]
    want, wops = M.asm_extend(ctx, bvol, qvol, jobs, cap)
    longest = int(want[:, 0].max())
    assert longest > 1000

    def good():
        d, o = M.asm_extend(ctx, bvol, qvol, jobs, cap)
        assert np.array_equal(d, want) and np.array_equal(o, wops)

    with pytest.raises(M.MhipError, match="multiple of 16"):
        M.asm_extend(ctx, bvol, qvol, jobs, cap + 8)
    good()
    with pytest.raises(M.MhipError, match="more than dir_cols_cap"):
        M.asm_extend(ctx, bvol, qvol, jobs, (longest // 16) * 16 - 16)
    good()
    with pytest.raises(M.MhipError, match="more than dir_cols_cap"):
        M.asm_extend_run(ctx, bvol, qvol, jobs, (longest // 16) * 16 - 16)
    good()
    for field, value in (("lx", int(bvol.offs[jobs[0]["xid"], 1])), ("ry", int(qvol.offs[jobs[0]["yid"], 1])), ("rx", -1), ("xid", bvol.num_reads)):
        bad = jobs.copy()
        bad[0][field] = value
        with pytest.raises(M.MhipError, match="extension job 0"):
            M.asm_extend(ctx, bvol, qvol, bad, cap)
        good()
    total = M.asm_extend_run(ctx, bvol, qvol, jobs, cap)
    with pytest.raises(M.MhipError, match="mhip_asm_extend_fetch"):
        M.asm_extend_fetch(ctx, len(jobs) - 1, total)
    d, offs, dense = M.asm_extend_fetch(ctx, len(jobs), total)
    check_dense(want, wops, d, offs, dense, total)
    good()
    bvol.free(); qvol.free(); ctx.close()
