"""The single-workgroup array scan (mecat_amd/csrc/scan.h: scan_array_1024) that every count-to-position kernel of the pipeline calls:
tiles of 1 024 with a running sum.  mhip_debug_scan runs it through cns_plan_scan (int32 counts, 64-bit sums, a base) with lengths on and
around the wave (64) and tile (1 024, 2 048) edges, where a carry goes wrong if it ever does; then dw_job_scan, the 32-bit wrapper whose
stage can be given any array length (mhip_jobs_from_candidates_dev), against the job order computed in numpy.  The other wrappers'
length-edge tests live with their stages: ae_word_offsets in test_gpu_asm_extend.py, cns_pieces_scan in test_gpu_cns_pieces.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 5000]
I32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ctx():
    import mecat_amd.hip as M
    c = M.Context(0)
    yield c
    c.close()


def values(kind, n):
    if kind == "random":
        return np.random.default_rng(1024 + n).integers(0, I32_MAX, n, dtype=np.int64, endpoint=True).astype(np.int32)
    return np.full(n, I32_MAX, np.int32)                    # the sum passes 2^32 from n = 3 on


@pytest.mark.parametrize("kind", ["random", "all_max"])
@pytest.mark.parametrize("base", [0, 2 ** 40])
@pytest.mark.parametrize("n", LENGTHS)
def test_scan_equals_cumsum(ctx, n, base, kind):
    import mecat_amd.hip as M
    cnt = values(kind, n)
    want = base + np.concatenate([np.zeros(1, np.int64), np.cumsum(cnt, dtype=np.int64)])
    got = M.debug_scan(ctx, cnt, base)
    assert got.dtype == np.int64 and len(got) == n + 1
    assert np.array_equal(got, want), "n %d: first difference at entry %d" % (n, int(np.nonzero(got != want)[0][0]))


def test_negative_length_is_refused_and_the_context_stays_usable(ctx):
    import mecat_amd.hip as M
    cnt = values("random", 1025)
    with pytest.raises(M.MhipError):
        M.debug_scan(ctx, cnt, 0, n=-1)
    want = 5 + np.concatenate([np.zeros(1, np.int64), np.cumsum(cnt, dtype=np.int64)])
    assert np.array_equal(M.debug_scan(ctx, cnt, 5), want)


@pytest.mark.parametrize("part_count", [1, 3])
@pytest.mark.parametrize("n_reads", [1, 1024, 1025, 2049])
def test_job_list_across_the_scan_tiles(ctx, n_reads, part_count):
    """dw_job_scan: one read, a whole tile, a tile and one read, two tiles and one read — 0 .. 4 candidates a read.  Job g of the
    read-major order goes to part g % part_count, slot g // part_count; a part's count is its share of the total."""
    import torch
    import mecat_amd.hip as M
    from mecat_amd import workload as W
    maxc, rid_begin, ref_start = 4, 7, 3
    rng = np.random.default_rng(n_reads)
    counts = rng.integers(0, maxc + 1, n_reads).astype(np.int32)
    counts[0] = maxc                                          # (a list is never empty)
    raw = rng.integers(0, 50000, (n_reads, maxc, 12)).astype(np.int32)
    raw[..., :2][rng.random((n_reads, maxc, 2)) < 0.2] = 0    # loc1 / loc2 == 0: no half-k-mer shift
    cands = raw.view(M.CAND_DTYPE).reshape(n_reads, maxc)
    want = W.jobs_from_candidates(cands, counts, rid_begin, ref_start)
    assert len(want) == int(counts.sum())
    dev = torch.device("cuda", 0)
    d_cands, d_counts = torch.from_numpy(raw).to(dev), torch.from_numpy(counts).to(dev)
    for part in range(part_count):
        d_jobs = torch.full((len(want), 5), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        nj = M.jobs_from_candidates_dev(ctx, d_cands.data_ptr(), d_counts.data_ptr(), n_reads, maxc, rid_begin, 1, ref_start, part, part_count, d_jobs.data_ptr())
        mine = want[part::part_count]
        assert nj == len(mine)
        got = d_jobs.cpu().numpy()
        assert np.array_equal(got[:nj], np.stack([mine[f] for f in M.JOB_DTYPE.names], axis=1)), "part %d of %d" % (part, part_count)
        assert (got[nj:] == -1).all()
