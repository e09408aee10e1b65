#!/usr/bin/env python3
"""Golden vectors for the corrected reads (mecat_amd/csrc/cns_reads.hip, csrc/cns_reads.h): what the UNMODIFIED back end of mecat2cns —
meap_add_one_aln, add_aln, get_effective_ranges and consensus_worker (mecat2cns/mecat_correction.cpp) — pushes into cns_results for one
template, through cns_reads_ref_main.cpp next to this file, compiled into a temporary directory against the reference's headers where
they lie and linked with oracle/_ref/libref_cns_table.so.  Build container only:
    python tests/golden/make_golden_cns_reads.py
Writes tests/golden/cns_reads.npz, inputs and recorded results only (tests/cns_reads_ref.py save_fixture / load_fixture): the hand-written
edge cases, N_RANDOM seeded random templates and the generated long cases around output_cns_result's block rule (their inputs as
generator parameters, their sequences as SHA-256).  Prints the census the CPU test asserts."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cns_reads_ref as R  # noqa: E402


def census(cases, results):
    """what the recorded results show: cases with a read, records, cut segments, and the arms of the range[1] rule among the records of
    cut segments (R + beg, `end` in the last block, `end` in a block that is not the last)"""
    count = dict(cases=len(cases), with_read=0, records=0, cut_records=0, arm_r_plus_beg=0, arm_end_last=0, arm_end_inner=0, longer=0, shorter=0)
    for c, row in zip(cases, results):
        count["with_read"] += len(row) > 0
        count["records"] += len(row)
        if c["long"] is None:
            continue
        sizes = [len(r[3]) if len(r) == 4 else r[3] for r in row]
        assert len(row) >= 1
        beg, end = row[0][1], row[-1][2]
        total = sizes[-1] + 39000 * (len(row) - 1)
        count["longer"] += total > end - beg
        count["shorter"] += total < end - beg
        if len(row) > 1:
            count["cut_records"] += len(row)
            for k, r in enumerate(row):
                last = k == len(row) - 1
                count["arm_end_last"] += last
                count["arm_end_inner"] += (not last) and r[2] == end
                count["arm_r_plus_beg"] += (not last) and r[2] != end
    return {k: int(v) for k, v in count.items()}


def main():
    cases = R.fixture_cases()
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_ref_program(tmp)
        results = R.run_ref(exe, cases, tmp)
    R.save_fixture(R.FIXTURE, cases, results)
    R._fixture = None
    cases2, rows = R.load_fixture()
    differ = 0
    for c, row in zip(cases2, rows):
        h = R.host_back_end(c)
        differ += not R.same_as_recorded(R.results_of(h["reads"], h["seq"]), row)
    print("bytes", os.path.getsize(R.FIXTURE), file=sys.stderr)
    print("the host back end + restatement differ on", differ, "cases", file=sys.stderr)
    print(census(cases2, rows), file=sys.stderr)


if __name__ == "__main__":
    main()
