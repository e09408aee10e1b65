"""mecat2ref's extension stage without a device: the restatement tests/ref_ext_ref.py and the host side mecat_amd/host/ref_results.cpp +
ref_reads.cpp (through tests/ref_results_lib.cpp) against what the UNMODIFIED extend_candidate recorded (tests/golden/ref_ext.npz,
tests/golden/make_golden_ref_ext.py)."""
import json
import zlib

import numpy as np
import pytest

import ref_cand_cases as RC
import ref_ext_cases as XC
import ref_ext_ref as X


@pytest.fixture(scope="module")
def fx():
    return XC.fixture()


@pytest.fixture(scope="module")
def restated(fx):
    """the restatement's result for every candidate of the fixture, once"""
    return [X.extend(fx["ref_codes"], fx["read_list"][int(c[0])], int(c[1]), int(c[2]), int(c[3])) for c in fx["cands"]]


def test_fixture_holds_the_cases_it_was_made_for(fx):
    shown = json.loads(str(fx["asserted"]))
    assert shown["candidates"][:2] == [575, 1060] and shown["candidates"][2] >= 100
    assert len(fx["cands"]) == sum(shown["candidates"]) == len(fx["res"]) == len(fx["crc"])
    for k in ("dirs_one_block", "dirs_several_blocks", "dirs_last_block_sized", "dirs_best_point", "dirs_tail_over_16_rows", "empty_left_ok",
              "clipped_first_base", "clipped_last_base", "across_chromosomes", "across_n_run", "lower_case_and_n_on_reverse", "under_1000"):
        assert shown[k] >= 1, k
    assert min(shown["ok_by_chain"]) >= 20
    # the recorded lists are ref_cand.npz's, in call order
    base = RC.fixture()
    at = 0
    for rnd in (1, 2):
        for rid, lst in enumerate(RC.recorded(base, 0, 10, rnd)):
            for c in lst:
                assert tuple(fx["cands"][at]) == (rid, c[9], c[0], c[1], c[6]) and fx["source"][at] == rnd
                at += 1
    assert at == 575 + 1060 and (fx["source"][at:] == 0).all()


def test_restatement_equals_the_tool(fx, restated):
    for i, (w, want, dirs) in enumerate(zip(restated, fx["res"], fx["dirs"])):
        got = tuple(w[k] for k in XC.RES_FIELDS)
        assert got == tuple(int(x) for x in want), (i, got, want)
        for side, f, cols in ((0, w["left"], w["lcols"]), (1, w["right"], w["rcols"])):
            assert (cols, f["blocks"], f["sized_last"], f["fallback"], f["tail_rows"]) == tuple(int(x) for x in dirs[side]), (i, side)
        if w["ok"]:
            assert (zlib.crc32(w["qmap"]), zlib.crc32(w["smap"])) == tuple(int(x) for x in fx["crc"][i]), i


def test_stored_columns_are_the_strings_columns(fx, restated):
    for j, i in enumerate(fx["stored"]):
        w = restated[int(i)]
        words = fx["stored_words"][fx["stored_offs"][j]: fx["stored_offs"][j + 1]]
        assert np.array_equal(X.columns_of(w["qmap"], w["smap"]), words), i


def test_reads_packer_and_its_twin(fx):
    """ref_reads.cpp == the Python twin; against stage 1's packing the N plane is the same (ref_seed.hip skips a k-mer on the plane alone)
    and the codes differ only under the plane"""
    reads = fx["read_list"]
    a, b = XC.pack_reads(reads), XC.lib_pack_reads(reads)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    old = RC.pack_reads(reads)
    assert np.array_equal(old[1], a[1]) and np.array_equal(old[2], a[2]) and old[3] == a[3]
    diff = old[0] ^ a[0]
    assert diff.any() and not (diff & ~a[1]).any()
    # the strand rule on one read with every kind of letter
    r = np.frombuffer(b"ACGTacgtNnRyAC", dtype=np.uint8)
    assert X.ENCODE[X.strand_letters(r, 0)].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 0, 0, 0, 0, 1]
    assert X.ENCODE[X.strand_letters(r, 1)].tolist() == [2, 3, 0, 0, 0, 0, 3, 2, 1, 0, 0, 1, 2, 3]


def test_ref_results_rebuilds_strings_record_and_align_info(fx, restated):
    from mecat_amd import hip
    pac, npl, offs, _ = XC.pack_reads(fx["read_list"])
    g = RC.RefGenome(fx["ref_fasta"])
    seen = 0
    for j, i in enumerate(fx["stored"]):
        i = int(i)
        rid, chain, _, _, score = (int(x) for x in fx["cands"][i])
        w = restated[i]
        words = fx["stored_words"][fx["stored_offs"][j]: fx["stored_offs"][j + 1]]
        rec = np.zeros((), dtype=hip.REF_RESULT_DTYPE)
        for k in XC.RES_FIELDS:
            rec[k] = w[k]
        rec["chain"], rec["vscore"] = chain, score
        got = XC.lib_strings(rec, words, pac, npl, offs[rid, 0], g.pac)
        assert got is not None and (zlib.crc32(got[0]), zlib.crc32(got[1])) == tuple(int(x) for x in fx["crc"][i]), i
        assert got == (w["qmap"], w["smap"])
        want = b"%d\t%c\t%d\t%d\t%d\t%d\t%d\t%d\n%s\n%s\n" % (rid, b"FR"[chain], score, w["qb"], w["qe"], w["qs"], w["sb"], w["se"], w["qmap"], w["smap"])
        assert XC.lib_record(rid, rec, got[0], got[1]) == want
        assert XC.lib_align_info(rec, 3) == (w["qb"], w["qe"], -1, 3, -1, -1, 1, b"FR"[chain], w["sb"], w["se"])
        seen += chain
    assert seen >= 10 and len(fx["stored"]) - seen >= 10
    # a hand-over that does not add up is reported, not rebuilt
    bad = rec.copy()
    bad["qe"] -= 1
    assert XC.lib_strings(bad, words, pac, npl, offs[rid, 0], g.pac) is None
    g.free()
