"""mecat2ref's candidate stage without a GPU: the plain restatement (tests/ref_cand_ref.py) against the lists recorded from the unmodified
tool (tests/golden/ref_cand.npz, made by tests/golden/make_golden_ref_cand.py), and mecat_amd/host/ref_genome.cpp (the reference file
as volume, N plane, read table and chrindex.txt) against the recorded chrindex.txt and a numpy restatement."""
import ctypes as C
import json

import numpy as np
import pytest

import ref_cand_cases as RC
import ref_cand_ref as R


@pytest.fixture(scope="module")
def fx():
    return RC.fixture()


@pytest.fixture(scope="module")
def ref(fx):
    let, chrindex = R.read_reference(fx["ref_fasta"].tobytes())
    return let, chrindex, R.Index(let)


def test_fixture_shows_what_it_must(fx):
    a = json.loads(str(fx["asserted"]))
    assert min(a["chains"]) >= 20 and a["reads_with_2"] >= 1 and a["cut_at_3"] >= 1 and a["round2_differs"] >= 1 and a["loc1_below_1000"] >= 1
    assert a["reads"] == len(fx["read_list"]) >= 200
    groups = json.loads(str(fx["groups"]))
    lens = [len(r) for r in fx["read_list"]]
    assert {12, 13, 17, 999, 1000, 15000} <= set(lens) and max(lens) == 15000
    for tech, n in RC.RUNS:
        for rnd in (1, 2):
            rec = RC.recorded(fx, tech, n, rnd)
            assert len(rec) == len(lens)
            assert all(len(rec[r]) == 0 for r in groups["random"])
            assert all(len(x) <= n for x in rec)


@pytest.mark.parametrize("rnd", [0, 1])
def test_restatement_equals_the_recorded_lists(fx, ref, rnd):
    """every read, both technologies, both -n, field for field and in list order.  The candidates' arrival order does not depend on
    -n and, the tool never assigning its nanopore cutoff, not on the technology either: one stream per read and round serves the four runs."""
    idx = ref[2]
    assert RC.CUTOFF[0] == RC.CUTOFF[1]
    streams = [R.read_stream(idx, r, rnd, RC.CUTOFF[0]) for r in fx["read_list"]]
    for tech, n in RC.RUNS:
        rec = RC.recorded(fx, tech, n, rnd + 1)
        for i, (s, e) in enumerate(zip(streams, rec)):
            got = R.insert_list(s, n)
            assert got.shape == e.shape and (got == e).all(), (tech, n, rnd, i, got, e)


def test_ref_genome_chrindex_and_tables(fx, ref):
    let, chrindex, _ = ref
    assert chrindex == fx["chrindex"].tobytes()
    g = RC.RefGenome(fx["ref_fasta"].tobytes())
    assert g.chrindex == fx["chrindex"].tobytes()
    assert g.num_bases == len(let) and g.num_chroms == 3
    pac, nplane, table = R.ref_tables(let)
    assert (g.pac == pac).all() and (g.nplane == nplane).all()
    assert g.reads.shape == table.shape and (g.reads == table).all()
    # the table's runs are the maximal runs of A, C, G, T; together with the zero-length reads they mark exactly the 13-mers that hold
    # another letter: positions [end - 12, end] of every read end
    bad = R.kmer_ids(let) < 0
    marked = np.zeros(len(let) + 1, dtype=bool)
    for o, s in g.reads:
        marked[max(o + s - 12, 0): o + s + 1] = True
    assert (marked[: len(bad)] == bad).all() and marked[len(bad):].all()
    assert (np.diff(g.reads[:, 0]) > 0).all() and (g.reads[:, 1] == 0).sum() >= 5
    g.free()


@pytest.mark.parametrize("text,chrindex,reads", [
    (b">a\nACGT\n", b"0\ta\t4\n4\tFileEnd\n", [(0, 4)]),
    (b">a b\r\nNNACGTN\r\n>c\td\nacgtR", b"0\ta\t7\n7\tc\t5\n12\tFileEnd\n", [(0, 0), (1, 0), (2, 4), (7, 4)]),
    (b">e\n>f\nAC\n", b"0\te\t0\tf\t2\n2\tFileEnd\n", [(0, 2)]),          # an empty record writes no size, as in the tool
    (b">n\n" + b"N" * 40 + b"A\n", b"0\tn\t41\n41\tFileEnd\n", [(0, 0), (13, 0), (26, 0), (39, 0), (40, 1)]),
])
def test_ref_genome_hand_cases(text, chrindex, reads):
    g = RC.RefGenome(text)
    assert g.chrindex == chrindex
    assert [tuple(r) for r in g.reads.tolist()] == reads
    let, ci = R.read_reference(text)
    pac, nplane, table = R.ref_tables(let)
    assert ci == chrindex and (g.pac == pac).all() and (g.nplane == nplane).all() and (g.reads == table).all()
    g.free()


def test_ref_genome_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError, match="no FASTA record"):
        RC.RefGenome(b"ACGT\n")
    with pytest.raises(ValueError, match="without a name"):
        RC.RefGenome(b">\nACGT\n")
    with pytest.raises(ValueError, match="no sequence letters"):
        RC.RefGenome(b">a\n\n")


def test_struct_sizes():
    from mecat_amd import hip
    assert C.sizeof(hip.RefCandidate) == 64 == hip.REF_CAND_DTYPE.itemsize
    assert C.sizeof(hip.RefSeedParams) == 16
    assert hip.RefCandidate.score.offset == 48 and hip.RefSeedParams.ddfs_cutoff.offset == 8
    p = hip.ref_seed_params(1)
    assert (p.maxc, p.round, p.ddfs_cutoff) == (10, 0, 0.25)
