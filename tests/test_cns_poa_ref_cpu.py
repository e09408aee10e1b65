"""The POA window routine (mecat_amd/csrc/cns_poa.h, compiled for the host as libcns_poa_host.so) against what the unmodified
meap_cns_one_indel returned for the cases of tests/golden/cns_poa.npz, and the C ABI of the POA entry points.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cns_poa_cases as P

ROOT = P.ROOT

# every situation at least 20 times in the fixture (one count per window that shows it).  stops_early — a best path that ends before '$'
# — is not in the list: the generator cannot reach one, and neither can any input of meap_cns_one_indel.  Every addAln ends with an
# edge into '$' and every vertex it makes gets an out-edge, the merges only move edges between vertices that keep one, so '$' is the only
# vertex with edges and no out-edge; bestPath's backwards FIFO then reaches every vertex that has an edge and gives it a best edge.  The
# fixture's count is printed and asserted to be 0.
NEED = dict.fromkeys([s for s in P.SITUATIONS if s != "stops_early"], 20)


@pytest.fixture(scope="module")
def host_results():
    """the host routine on every fixture case, once: [(pieces, piece_begin, strings, info)]"""
    cases, _ = P.load_fixture()
    out = []
    for c in cases:
        pieces, pb = P.pieces_of(c)
        got, info = P.host_run(c, pieces, pb)
        out.append((pieces, pb, got, info))
    return out


def test_host_routine_equals_the_reference(host_results):
    cases, strings = P.load_fixture()
    assert len(cases) > 1500 and sum(len(c["windows"]) for c in cases) > 5000
    for i, (c, want, (_, _, got, _)) in enumerate(zip(cases, strings, host_results)):
        assert got == want, (i, c["windows"], [(g, w) for g, w in zip(got, want) if g != w][:3])


def test_thresholds():
    """(int)(cov * 0.4) for cov 0 .. 255 as the reference computes it, read off the two threshold cases' recorded strings.  The first
    graph's path has the weights 101, 101, 100, .. 2: a string of n letters means a threshold of 103 - n (n == 101: at most 2; 0: 102 or
    more).  The second graph has weight 1 only: letters mean a threshold of at most 1, none 2 or more."""
    cases, strings = P.load_fixture()
    k = [i for i, c in enumerate(cases) if c["fresh"]]
    assert len(k) == 2 and all([w[2] for w in cases[i]["windows"]] == list(range(256)) for i in k) and len(cases[k[0]]["alns"]) == 100 and not cases[k[1]]["alns"]
    L = P.host_lib()
    seen = set()
    for cov, (s, e) in enumerate(zip(strings[k[0]], strings[k[1]])):
        m, n = L.cns_poa_host_min_weight(cov), len(s)
        assert s == b"A" * n and e in (b"", b"NNNNNN")
        want = {0, 1, 2} if n == 101 else ({102} if n == 0 else {103 - n})
        want &= {0, 1} if e else set(range(2, 103))
        assert want == ({0, 1} if e else {m}) and m in want and m == int(cov * 0.4), (cov, n, e, m)
        seen.add(m)
    assert seen == set(range(103))          # cov 255 reaches 102


def test_census(host_results):
    cases, strings = P.load_fixture()
    count = dict.fromkeys(P.SITUATIONS, 0)
    for c, row, (pieces, pb, _, info) in zip(cases, strings, host_results):
        P.census(c, pieces, pb, row, info, count)
    print({k: int(v) for k, v in count.items()})
    for k, v in NEED.items():
        assert count[k] >= v, (k, int(count[k]), v)
    assert count["stops_early"] == 0


def test_workspace_stays_within_the_stated_bound(host_results):
    """nodes, edges, queue entries, frames and members against the header's CAPACITIES: blen + 2 + insertion columns nodes, blen + 1 +
    addEdge calls edges, computed here from the strings, not taken from the library"""
    cases, _ = P.load_fixture()
    col = {n: i for i, n in enumerate(P.INFO_NAMES)}
    top = dict.fromkeys(("nodes", "edges", "queue", "frames", "members"), 0.0)
    for c, (pieces, pb, got, info) in zip(cases, host_results):
        for w, (sb, se, _) in enumerate(c["windows"]):
            ins = calls = 0
            for p in pieces[pb[w]: pb[w + 1]]:
                q, s, _, _ = c["alns"][int(p["aln"])]
                a, n = int(p["col"]), int(p["ncols"])
                qq, ss = np.frombuffer(q[a: a + n], np.uint8), np.frombuffer(s[a: a + n], np.uint8)
                i = int(((qq != P.GAP) & (ss == P.GAP)).sum())
                ins += i
                calls += i + int(((qq == ss) & (qq != P.GAP)).sum()) + 1
            nodes, edges = se - sb + 1 + 2 + ins, se - sb + 1 + 1 + calls
            r = info[w]
            assert r[col["rc"]] == 0 and r[col["bound_nodes"]] == nodes and r[col["bound_edges"]] == edges, (c["windows"][w], r)
            assert r[col["nodes"]] == nodes and r[col["edges"]] <= edges
            assert r[col["queue"]] <= nodes and r[col["frames"]] <= nodes and r[col["members"]] <= nodes and len(got[w]) <= nodes - 2
            for k in top:
                top[k] = max(top[k], r[col[k]] / (edges if k == "edges" else nodes))
    print({k: round(v, 3) for k, v in top.items()})
    assert top["edges"] == 1.0          # the edge bound is met, not just respected


def test_abi():
    """both libraries export the entry points; the sizes the tests rely on; the WANT bit and the prototype compile from the header"""
    import mecat_amd.hip as M
    L = C.CDLL(M.lib_path())
    assert L.mhip_cns_accept_templates_poa and L.mhip_debug_cns_poa and L.mhip_cns_poa_small_words
    assert M.CNS_WANT_POA == 16
    H = P.host_lib()
    assert H.cns_poa_host_case and H.cns_poa_host_info_words() == len(P.INFO_NAMES) and H.cns_poa_host_stats_bytes() == 4 * (len(P.INFO_NAMES) - 3)
    assert H.cns_poa_host_words(10, 20) == 17 * 10 + 8 * 20
    L.mhip_cns_poa_small_words.restype = C.c_int64
    assert L.mhip_cns_poa_small_words() >= H.cns_poa_host_words(4, 3)          # the smallest window (blen 2, no piece) fits the small slot
    src = ('#include "mecat_hip.h"\n_Static_assert(MHIP_CNS_WANT_POA == 16, "bit");\n_Static_assert(sizeof(mhip_cns_window) == 16, "window");\n'
           'int (*f)(mhip_ctx*, const mhip_volume*, mhip_ext_candidate*, const int64_t*, int, int, int, double, int, int, int, int, mhip_cns_accepted**, int64_t*, char**, '
           'int64_t*, int64_t*, mhip_cns_table_item**, uint8_t**, int64_t**, mhip_cns_segment**, int64_t**, mhip_cns_window**, int64_t*, int32_t**, int64_t**, '
           'mhip_cns_piece**, int64_t**, char**, int64_t**) = mhip_cns_accept_templates_poa;\n')
    r = subprocess.run(["cc", "-x", "c", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    # the header of the routine compiles as plain C++ without HIP
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mecat_amd", "csrc"), "-x", "c++", "-"],
                       input=b'#include "cns_poa.h"\n', capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


@pytest.mark.ref
@pytest.mark.skipif(not P.have_reference(), reason="the reference and oracle/_ref exist in the build container only")
def test_fresh_random_cases_against_the_reference(tmp_path):
    """2 000 cases from a second seed through the reference's program and the host routine"""
    cases = P.random_cases(P.FRESH_SEED, 2000)
    want = P.run_ref(P.build_ref_program(tmp_path), cases, tmp_path)
    nwin = 0
    for i, (c, row) in enumerate(zip(cases, want)):
        got, _ = P.host_run(c)
        assert got == row, (i, c["windows"], [(g, w) for g, w in zip(got, row) if g != w][:3])
        nwin += len(row)
    print("windows", nwin)
    assert nwin > 5000
