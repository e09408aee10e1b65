"""The corrected reads on the host (tests/cns_reads_ref.py): the literal restatement of meap_consensus_one_segment's target, the size
filter and output_cns_result — over the host back end (table, plan, piece cursor, libcns_poa_host.so's window routine) — against what the
unmodified consensus_worker recorded in tests/golden/cns_reads.npz, and csrc/cns_reads.h's split function, exported from
libcns_poa_host.so (the code the record kernel runs), against both.  Where the compiled reference is available the driver runs again on
fresh seeded cases."""
import importlib.util
import os

import pytest

import cns_reads_ref as R

_spec = importlib.util.spec_from_file_location("make_golden_cns_reads", os.path.join(R.GOLDEN, "make_golden_cns_reads.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)


def test_fixture_is_what_the_generators_give():
    cases, rows = R.load_fixture()
    fresh = R.fixture_cases()
    assert len(cases) == len(fresh) == len(rows)
    for a, b in zip(cases, fresh):
        assert a == b
    assert os.path.getsize(R.FIXTURE) < 1 << 20


def test_census():
    cases, rows = R.load_fixture()
    c = MG.census(cases, rows)
    assert c == {'cases': 222, 'with_read': 207, 'records': 214, 'cut_records': 11, 'arm_r_plus_beg': 5, 'arm_end_last': 5, 'arm_end_inner': 1, 'longer': 1, 'shorter': 1}
    # the five sizes around the block rule, as the reference cut them
    longs = [(x, row) for x, row in zip(cases, rows) if x["long"] is not None and x["long"][0] == 0]
    assert [x["long"][1] for x, _ in longs] == list(R.LONG_SIZES)
    assert [[r[3] for r in row] for _, row in longs] == [[59999], [60000], [49000, 21001], [49000, 60000], [49000, 49000, 21001]]
    random = [row for x, row in zip(cases, rows) if x["long"] is None][-R.N_RANDOM:]
    assert sum(len(row) > 0 for row in random) > 0.9 * R.N_RANDOM


def test_restatement_against_the_reference():
    cases, rows = R.load_fixture()
    for i, (c, row) in enumerate(zip(cases, rows)):
        h = R.host_back_end(c)
        assert R.same_as_recorded(R.results_of(h["reads"], h["seq"]), row), i
        assert R.format_reads(h["reads"], h["seq"]).count(b">") == len(row)


def test_split_function():
    """the exported function: the fixture's record lists, and the restatement for every size from 1 to 200 000"""
    cases, rows = R.load_fixture()
    for c, row in zip(cases, rows):
        if c["long"] is None or not row:
            continue
        beg, end = row[0][1], row[-1][2]
        sizes = [r[3] for r in row]
        total = sizes[-1] + 39000 * (len(row) - 1)
        got = R.host_split(total, beg, end)
        assert [(r0, r1, Rr - L) for L, Rr, r0, r1 in got] == [(r[1], r[2], r[3]) for r in row]
    import ctypes as C
    lib = R.P.host_lib()
    R.host_split(1, 0, 1)                                   # (sets the argument types)
    o = (C.c_int64 * 4)()
    for size in range(1, 200001):
        want = R.split(size, 11, 11 + 70000)
        n = lib.cns_reads_host_blocks(size)
        assert n == len(want), size
        if size > R.MAX_SEQ - 2 or size % 997 == 0:
            for k in range(n):
                lib.cns_reads_host_block(size, k, 11, 11 + 70000, o)
                assert tuple(o) == want[k], (size, k)
    for size, beg, end in ((60001, 0, 10), (200000, 5, 100000), (200000, 5, 300000), (120000, 0, 88000), (120000, 0, 88001)):
        assert R.host_split(size, beg, end) == R.split(size, beg, end)


@pytest.mark.skipif(not R.have_reference(), reason="the compiled reference is not available")
def test_fresh_cases_against_the_compiled_reference(tmp_path):
    cases = R.random_cases(R.FRESH_SEED, 60) + [R.long_case(1, 52000, 300), R.long_case(0, 138001, 301)]
    exe = R.build_ref_program(tmp_path)
    rows = R.run_ref(exe, cases, tmp_path)
    assert sum(len(r) > 0 for r in rows) > 50
    for i, (c, row) in enumerate(zip(cases, rows)):
        h = R.host_back_end(c)
        assert R.results_of(h["reads"], h["seq"]) == [tuple(r) for r in row], i
