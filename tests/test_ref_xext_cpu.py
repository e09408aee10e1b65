"""mecat2ref's extension stage in nanopore mode, the parts that need no GPU: the C ABI exports the new calls, tests/golden/ref_xext.npz
holds the cases it was made for, oracle/liboracle.so's orc_xdrop_go on tests/ref_ext_ref.py's windows and strand codes equals what the
unmodified extend_candidate recorded with an XdropAligner (which pins the expected value tests/test_gpu_ref_xextend.py uses for fresh
cases), the stored columns rebuild the CRC'd strings, and mecat_amd/host/ref_results.cpp rebuilds text, record and AlignInfo of results
whose code-0 columns hold different letters."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import helpers as H
import ref_cand_cases as RC
import ref_ext_cases as XC
import ref_ext_ref as X
import ref_rescue_cases as SC
import ref_xext_cases as XX

NEW = ("mhip_ref_xextend_run", "mhip_ref_xextend_run_dev", "mhip_ref_xextend_stats", "mhip_ref_xrescue_run", "mhip_ref_xrescue_run_dev")


@pytest.fixture(scope="module")
def fx():
    return XX.fixture()


def test_the_new_symbols_are_exported_declared_and_mirrored():
    subprocess.run(["make", "-s", "hip"], cwd=H.ROOT, check=True, stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(H.ROOT, "mecat_amd", "lib", "libmecat_hip.so"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "mecat_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mhip_[a-z_0-9]+)\s*\(", hdr))
    mirror = open(os.path.join(H.ROOT, "mecat_amd", "hip.py")).read()
    doc = open(os.path.join(H.ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert "lib()." + name in mirror, name
        assert name in doc, name


def test_fixture_holds_the_cases_it_was_made_for(fx):
    shown = fx["asserted"]
    n = len(fx["cands"])
    assert n == sum(shown["candidates"]) == len(fx["res"]) == len(fx["crc"]) == len(fx["dirs"]) == len(fx["set"]) == len(fx["source"])
    assert shown["candidates"][:2] == [575, 1060] and shown["natural"] == 2023 and shown["recorded"] == 1635
    res, dirs, nat, src = fx["res"].astype(np.int64), fx["dirs"].astype(np.int64), fx["set"] == 0, fx["source"]
    ok = res[:, 0] == 1
    span = res[:, 2] - res[:, 1]
    assert (ok == (span >= XX.MIN_SPAN)).all()          # the query span decides, not the columns
    assert (res[:, 6] == np.maximum(dirs[:, 0, 0] - 1, 0) + dirs[:, 1, 0]).all()          # the left half joins without its last column
    assert ((fx["crc"] != 0).all(axis=1) == ok).all()
    for chain in (0, 1):
        assert (ok & nat & (fx["cands"][:, 1] == chain)).sum() >= 100
    assert (~ok & nat & (res[:, 6] > 0)).sum() >= 20
    assert (nat & (res[:, 6] >= 1000) & (span < 1000)).sum() >= 10
    assert (nat & (span >= 990) & (span <= 1010)).sum() >= 5
    assert (dirs[nat][:, :, 3] == 1).sum() >= 100          # directions ended by X-drop
    assert (nat & (dirs[:, 0, 0] == 1)).sum() >= 5          # one-column left halves
    assert (nat & ok & (dirs[:, 0, 0] == 0)).sum() >= 1          # an empty left half that is ok
    assert (dirs[:, :, 4] == 1).sum() >= 1 and ((dirs[:, :, 4] == 1) & (dirs[:, :, 1] == 2)).sum() >= 1          # failed trims, one in a second block
    assert (ok & (src == XX.SRC_LOWC)).sum() >= 1
    for k in ("clipped_first_base", "clipped_last_base", "across_chromosomes", "across_n_run", "lower_case_and_n_on_reverse"):
        assert shown[k] >= 1, k
    # the stored subset: every ok result off the recorded lists, a share of those
    stored = set(int(i) for i in fx["stored"])
    assert all(ok[i] for i in stored) and all(int(i) in stored for i in np.flatnonzero(ok & ~np.isin(src, (1, 2))))
    assert sum(1 for i in stored if src[i] in (1, 2)) >= 100
    assert os.path.getsize(XX.FIXTURE) <= os.path.getsize(os.path.join(H.GOLDEN, "ref_cand.npz"))
    # the inputs are the ones the generator derives: the recorded lists, the hand-made candidates' count, the second set
    base = RC.fixture()
    at = 0
    for rnd in (1, 2):
        for rid, lst in enumerate(RC.recorded(base, 1, 10, rnd)):
            for c in lst:
                assert tuple(int(x) for x in fx["cands"][at]) == (rid, int(c[9]), int(c[0]), int(c[1]), int(c[6])) and src[at] == rnd
                at += 1
    assert at == 1635
    _, _, cands1, source1 = XX.second_set()
    assert np.array_equal(fx["cands"][~nat], cands1) and np.array_equal(src[~nat], source1)


def test_the_rescue_chain_runs_show_their_cases(fx):
    seen = fx["asserted"]["tool"]
    for k in ("early_return", "left_attach", "right_attach", "extended_not_attached"):
        assert seen[k] >= 1, (k, seen)
    codes = fx["sets"][0]["ref_codes"]
    extra = XX.extra_chain_reads(codes)
    assert len(extra) == len(fx["tool_extra_reads"]) and all(np.array_equal(a, b) for a, b in zip(extra, fx["tool_extra_reads"]))
    n = len(XX.chain_reads())
    for nb in XX.TOOL_RUNS:
        calls = fx["tool"][nb]
        assert {c["read"] for c in calls} == set(range(n))
        assert sum(1 for c in calls for a in c["after"] if a[6] != -1) >= 1 and sum(1 for c in calls for a in c["after"] if a[7] != -1) >= 1


@pytest.fixture(scope="module")
def oracle_results(fx):
    out = []
    for i, c in enumerate(fx["cands"]):
        s = fx["sets"][int(fx["set"][i])]
        out.append(XX.xgo(s["ref_codes"], s["read_list"][int(c[0])], int(c[1]), int(c[2]), int(c[3])))
    return out


def test_the_oracle_equals_the_tool_on_every_candidate(fx, oracle_results):
    for i, (w, want) in enumerate(zip(oracle_results, fx["res"])):
        got = tuple(w[k] for k in XX.RES_FIELDS)
        assert got == tuple(int(x) for x in want), (i, got, want)


def test_stored_columns_rebuild_the_strings(fx):
    for j, i in enumerate(fx["stored"]):
        i = int(i)
        s = fx["sets"][int(fx["set"][i])]
        rid, chain = int(fx["cands"][i][0]), int(fx["cands"][i][1])
        _, qb, qe, _, sb, se, cols, matches = (int(x) for x in fx["res"][i])
        words = fx["stored_words"][fx["stored_offs"][j]: fx["stored_offs"][j + 1]]
        assert len(words) == (cols + 15) // 16
        strand = X.ENCODE[X.strand_letters(s["read_list"][rid], chain)]
        qm, sm, qe2, se2 = X.strings_of(words, cols, strand, s["ref_codes"], qb, sb)
        assert (qe2, se2) == (qe, se) and (zlib.crc32(qm), zlib.crc32(sm)) == tuple(int(x) for x in fx["crc"][i]), i
        a, b = np.frombuffer(qm, dtype=np.uint8), np.frombuffer(sm, dtype=np.uint8)
        assert int((a == b).sum()) == matches and np.array_equal(XX.columns_of(qm, sm), words)


def test_ref_results_rebuilds_results_with_mismatch_columns(fx):
    """text, temporary-result record and AlignInfo entry from columns whose code 0 stands over unequal letters"""
    from mecat_amd import hip
    seen = dict(mismatch_columns=0, rev=0, fwd=0)
    for k in (0, 1):
        s = fx["sets"][k]
        pac, npl, offs, _ = XC.pack_reads(s["read_list"])
        g = RC.RefGenome(s["ref_fasta"])
        for j, i in enumerate(fx["stored"]):
            i = int(i)
            if fx["set"][i] != k:
                continue
            rid, chain, _, _, score = (int(x) for x in fx["cands"][i])
            words = fx["stored_words"][fx["stored_offs"][j]: fx["stored_offs"][j + 1]]
            rec = np.zeros((), dtype=hip.REF_RESULT_DTYPE)
            for f, v in zip(XX.RES_FIELDS[:7], fx["res"][i]):
                rec[f] = v
            rec["chain"], rec["vscore"] = chain, score
            got = XC.lib_strings(rec, words, pac, npl, offs[rid, 0], g.pac)
            assert got is not None and (zlib.crc32(got[0]), zlib.crc32(got[1])) == tuple(int(x) for x in fx["crc"][i]), i
            a, b = np.frombuffer(got[0], dtype=np.uint8), np.frombuffer(got[1], dtype=np.uint8)
            seen["mismatch_columns"] += int(((a != b) & (a != 45) & (b != 45)).sum())
            qb, qe, qs, sb, se = (int(rec[f]) for f in ("qb", "qe", "qs", "sb", "se"))
            want = b"%d\t%c\t%d\t%d\t%d\t%d\t%d\t%d\n%s\n%s\n" % (rid, b"FR"[chain], score, qb, qe, qs, sb, se, got[0], got[1])
            assert XC.lib_record(rid, rec, got[0], got[1]) == want
            assert XC.lib_align_info(rec, 3) == (qb, qe, -1, 3, -1, -1, 1, b"FR"[chain], sb, se)
            seen["rev" if chain else "fwd"] += 1
        bad = rec.copy()
        bad["qe"] -= 1
        assert XC.lib_strings(bad, words, pac, npl, offs[rid, 0], g.pac) is None
        g.free()
    assert seen["mismatch_columns"] >= 1000 and seen["rev"] >= 10 and seen["fwd"] >= 10, seen
