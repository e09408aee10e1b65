"""The mecat2cns program's command line and the host rules of its m4 walk, without a GPU, against what the unmodified reference recorded
in tests/golden/cns_cli.npz (tests/golden/make_golden_cns_cli.py):
  - mecat_amd/bin/mecat2cns on every recorded argv vector: stdout, stderr and exit code of parse_arguments + print_options / print_usage;
  - the m4 rule set of mecat_amd/csrc/cns_replay.h (tests/cns_replay_m4_check.cpp, built here) on the recorded walks: fed the recorded
    result of GetAlignment for every overlap the reference looked at, it accepts what consensus_one_read_m4_* accepted, in its order;
  - hand cases of the rules, and of the driver's grouping and gates (mecat_amd/cns/cns_groups.h through tests/cns_groups_lib.cpp)."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import cns_cli_cases as CC
import helpers as H

BIN = os.path.join(H.ROOT, "mecat_amd", "bin", "mecat2cns")
G = np.load(os.path.join(H.GOLDEN, "cns_cli.npz"))
MAX_ADDED = {"pacbio": 60, "nanopore": 100}


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-s", "hip", "host"], cwd=H.ROOT, check=True, stdout=subprocess.DEVNULL)


# ---- the command line ------------------------------------------------------------------------------------------------------------------

CLI = json.loads(str(G["cli"]))


@pytest.mark.parametrize("k", range(len(CLI)), ids=[" ".join(c["argv"]) or "none" for c in CLI])
def test_command_line(k, tmp_path):
    c = CLI[k]
    r = subprocess.run(["mecat2cns"] + c["argv"], executable=BIN, capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.stdout.decode() == c["stdout"]
    assert r.stderr.decode() == c["stderr"]
    assert r.returncode == c["rc"]
    assert not os.listdir(str(tmp_path))          # options and usage are handled before anything is opened


def test_command_line_covers():
    """what the recording must hold: both technologies' defaults, every validation message, the three getopt refusals, -h, too few words"""
    err = "".join(c["stderr"] for c in CLI)
    for text in ("cpu threads must be greater than 0", "batch size must be greater than 0", "mapping ratio must be >= 0.0", "coverage must be >= 0", "sequence size must be >= 0",
                 "invalid argument to option 'i': 2", "unrecognised option 'z'", "unrecognised option 'c'", "USAGE:"):
        assert text in err, text
    out = [c["stdout"] for c in CLI]
    assert any("mapping ratio:\t0.9\n" in o and "tech:\t0\n" in o and "input_type:\t1\n" in o for o in out)
    assert any("mapping ratio:\t0.4\n" in o and "tech:\t1\n" in o and o.startswith("-x\n") for o in out)
    assert {c["rc"] for c in CLI} == {0, 1}


def test_x_as_the_last_word(tmp_path):
    """the stated difference: the reference reads behind argv there (options.cpp:168-173); here its message, the usage text, exit 1"""
    r = subprocess.run(["mecat2cns", "a", "b", "c", "-x"], executable=BIN, capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode().startswith("argument to option 'x' is missing.\nUSAGE:\nmecat2cns [options] input reads output\n")


# ---- the m4 rule set ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def m4_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("m4") / "cns_replay_m4_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(H.ROOT, "mecat_amd", "csrc"),
                    "-I" + os.path.join(H.ROOT, "include"), os.path.join(H.ROOT, "tests", "cns_replay_m4_check.cpp"), "-o", exe], check=True)
    return exe


def run_cases(exe, cases, tmp):
    """cases: (max_added, check_ratio, ratio, rows [n, 11]) -> per case (jobs, accepted record numbers, the order the walk left)"""
    path = os.path.join(str(tmp), "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for max_added, check, ratio, rows in cases:
            rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 11)
            f.write(struct.pack("<iidi", max_added, int(check), float(ratio), len(rows)))
            f.write(rows.tobytes())
    r = subprocess.run([exe, path], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr.decode()[-2000:]
    out = []
    for line in r.stdout.decode().splitlines():
        jobs, rest = line.split(":")
        acc, order = rest.split("|")
        out.append((int(jobs), [int(x) for x in acc.split()], [int(x) for x in order.split()]))
    assert len(out) == len(cases)
    return out


@pytest.mark.parametrize("name", ["pacbio", "nanopore"])
def test_m4_rules_on_the_recorded_walks(m4_check, tmp_path, name):
    key = name + "_m4"
    counts, seen, meta = G[key + "_walk_counts"], CC.table(key + "_walk_seen", 7), CC.table(key + "_walk_meta", 3)
    ratio = float(json.loads(str(G[name + "_opts"]))["-r"]) - 0.02
    cases, s0 = [], 0
    for nrec, looked, aligned, refused, nacc, nres in counts:
        assert looked == min(nrec, MAX_ADDED[name])
        rows = np.zeros((nrec, 11), np.int32)
        # the recorded records are in walk order already: strictly descending overlap sizes keep it (the records behind them are shorter)
        rows[:, 1] = 2000000 - np.arange(nrec)
        got = seen[s0: s0 + looked]
        rows[:looked, 4:6] = got[:, 5:7]
        rows[:looked, 6:11] = got[:, 0:5]
        rows[looked:, 6] = 1          # (would be accepted if the rules looked at them)
        rows[looked:, 7:11] = (0, 1000000, 0, 1000000)
        cases.append((MAX_ADDED[name], name == "nanopore", ratio, rows))
        s0 += looked
    assert s0 == len(seen)
    res = run_cases(m4_check, cases, tmp_path)
    m0 = 0
    for (nrec, looked, aligned, refused, nacc, nres), (jobs, acc, order), case in zip(counts, res, cases):
        assert jobs == looked and order == list(range(nrec))
        rows = case[3]
        assert [(int(rows[i, 9]), int(rows[i, 10])) for i in acc] == [(int(a), int(b)) for a, b, _ in meta[m0: m0 + nacc]]
        assert all(i < looked for i in acc)
        m0 += nacc
    assert m0 == len(meta)
    a = json.loads(str(G["asserted"]))[key]
    assert a["over_max"] >= 1 and a["upto_max"] >= 1 and a["align_failed"] >= 1 and (name == "pacbio" or a["ratio_refused"] >= 1)


def row(size, ok=1, qsize=10000, ssize=10000, oq=None, os_=None):
    """an overlap of that size (on the query), whose alignment covers oq letters of the query and os_ of the template"""
    oq = size if oq is None else oq
    os_ = size if os_ is None else os_
    return [0, size, 0, size - 1, qsize, ssize, ok, 0, oq, 0, os_]


@pytest.mark.parametrize("max_added", [60, 100])
def test_m4_rules_by_hand(m4_check, tmp_path, max_added):
    rng = np.random.default_rng(max_added)
    sizes = rng.permutation(np.arange(3000, 3000 + max_added + 1))
    exactly = [row(int(s)) for s in sizes[:max_added]]
    exactly[3][6] = 0                                              # an alignment that failed
    one_more = [row(int(s)) for s in sizes]
    one_more[int(np.argmax(sizes))][6] = 0
    ties = [row(5000) for _ in range(max_added - 10)] + [row(4000) for _ in range(30)] + [row(6000), row(3000)]
    # the template 10 000 long, the query 10 000: 5 000 of either is below 0.58 * 10 000, 5 800 is not
    ratio = [row(7000, oq=5000, os_=5000), row(7000, oq=5800, os_=100), row(7000, oq=100, os_=5800), row(7000, oq=5799, os_=5799), row(7000, ok=0)]
    cases = [(max_added, False, 0.58, exactly), (max_added, False, 0.58, one_more), (max_added, False, 0.58, ties), (max_added, False, 0.58, ratio), (max_added, True, 0.58, ratio)]
    res = run_cases(m4_check, cases, tmp_path)
    # exactly max_added: the order given, every record a job, the failed one left out
    jobs, acc, order = res[0]
    assert jobs == max_added and order == list(range(max_added)) and acc == [i for i in range(max_added) if i != 3]
    # one more: the whole range sorted by overlap size, descending; the first max_added are jobs; the largest failed, the smallest is not looked at
    jobs, acc, order = res[1]
    want = [int(i) for i in np.argsort(-sizes, kind="stable")]
    assert jobs == max_added and order == want and acc == want[1:max_added]
    # ties: no tie-break is promised — descending sizes, the same multiset, the largest first, the 3 000 never a job
    jobs, acc, order = res[2]
    got = [ties[i][1] for i in order]
    assert sorted(order) == list(range(len(ties))) and got == sorted(got, reverse=True) and jobs == max_added
    assert acc == order[:max_added] and got[0] == 6000 and got[:max_added].count(5000) == max_added - 10 and got[:max_added].count(4000) == 9
    # PacBio accepts where nanopore's ratio refuses
    assert res[3][1] == [0, 1, 2, 3] and res[4][1] == [1, 2]


# ---- the driver's grouping -------------------------------------------------------------------------------------------------------------

def test_groups_and_gates(tmp_path):
    so = str(tmp_path / "libcns_groups.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-I" + os.path.join(H.ROOT, "mecat_amd", "cns"), "-I" + os.path.join(H.ROOT, "include"),
                    os.path.join(H.ROOT, "tests", "cns_groups_lib.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.cns_groups_make.restype = C.c_int64
    L.cns_groups_make.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    # sid: records, ssize — min_cov 4, min_size 5000 (0.95 * 5000 = 4750)
    groups = {7: (4, 4750), 3: (3, 9000), 9: (6, 4749), 1: (5, 6000), 5: (4, 5000)}
    recs = []
    for sid, (n, ssize) in groups.items():
        for k in range(n):
            r = [0] * 13
            r[1], r[7], r[9], r[12] = 100 + k, sid, ssize, 1000 * sid + k
            recs.append(r)
    rng = np.random.default_rng(4)
    a = np.array(recs, np.int32)[rng.permutation(len(recs))].copy()
    tb, dropped = np.zeros(len(a) + 1, np.int64), np.zeros(2, np.int64)
    nt = L.cns_groups_make(a.ctypes.data, len(a), 4, 5000, tb.ctypes.data, dropped.ctypes.data)
    assert nt == 3 and dropped.tolist() == [1, 1] and tb[: nt + 1].tolist() == [0, 5, 9, 13]
    kept = a[: tb[nt]]
    assert kept[:, 7].tolist() == [1] * 5 + [5] * 4 + [7] * 4
    assert sorted(kept[:, 12].tolist()) == sorted(1000 * s + k for s in (1, 5, 7) for k in range(groups[s][0]))
