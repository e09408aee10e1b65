#!/usr/bin/env python3
"""Golden vectors for the POA windows' consensus (mecat_amd/csrc/cns_poa.h: the host build libcns_poa_host.so and the kernels of
cns_poa.hip): what the UNMODIFIED meap_cns_one_indel (mecat2cns/mecat_correction.cpp:62-78, AlnGraphBoost behind it) returns, through
cns_poa_ref_main.cpp next to this file — compiled into a temporary directory against the reference's headers where they lie and linked
with oracle/_ref/libref_cns_table.so.  Build container only:
    python tests/golden/make_golden_cns_poa.py
Writes tests/golden/cns_poa.npz, inputs and recorded results only (tests/cns_poa_cases.py save_fixture / load_fixture): the hand-written
cases, the two threshold cases (cov 0 .. 255 on graphs whose weights tell the values of (int)(cov * 0.4) apart) and N_RANDOM seeded random
cases; per window the string `cns`.  Prints the census the CPU test asserts."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cns_poa_cases as P  # noqa: E402

N_RANDOM = 1500


def fixture_cases():
    return P.hand_cases() + P.threshold_cases() + P.random_cases(P.FIXTURE_SEED, N_RANDOM)


def main():
    cases = fixture_cases()
    with tempfile.TemporaryDirectory() as tmp:
        exe = P.build_ref_program(tmp)
        strings = P.run_ref(exe, cases, tmp)
    P.save_fixture(P.FIXTURE, cases, strings)
    count = dict.fromkeys(P.SITUATIONS, 0)
    differ = 0
    for c, row in zip(cases, strings):
        pieces, pb = P.pieces_of(c)
        got, info = P.host_run(c, pieces, pb)
        differ += sum(g != r for g, r in zip(got, row))
        P.census(c, pieces, pb, row, info, count)
    print("cases", len(cases), "windows", sum(len(c["windows"]) for c in cases), "bytes", os.path.getsize(P.FIXTURE), file=sys.stderr)
    print("host routine differs on", differ, "windows", file=sys.stderr)
    print({k: int(v) for k, v in count.items()}, file=sys.stderr)


if __name__ == "__main__":
    main()
