"""What the tests of the mecat2cns program and of its m4 walk share (test_gpu_cns_cli.py, test_gpu_cns_text.py): the recorded runs of
tests/golden/cns_cli.npz as files a program can read, and the driver's own grouping of a partition file's records."""
import ctypes as C
import json
import lzma
import os
import subprocess

import numpy as np

import helpers as H

BIN = os.path.join(H.ROOT, "mecat_amd", "bin", "mecat2cns")
PARTITION = os.path.join(H.ROOT, "mecat_amd", "bin", "mecat2cns_partition")
MAX_ADDED = {"pacbio": 60, "nanopore": 100}
TECH = {"pacbio": 0, "nanopore": 1}
_fixture = None
_reads = {}
_groups = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(H.GOLDEN, "cns_cli.npz"))
    return _fixture


def table(key, cols):
    """an int32 table the generator stored as LZMA bytes of its columns (make_golden_cns_cli.py packed()) -> [n, cols]"""
    return np.frombuffer(lzma.decompress(fixture()[key].tobytes()), dtype=np.int32).reshape(cols, -1).T.copy()


def read_set(name):
    """the set regenerated from its seed -> (codes, lens)"""
    if name not in _reads:
        nr, L, Gn, seed, ont = (int(x) for x in fixture()[name + "_reads"])
        _reads[name] = H.synth_reads(nr, L, float(fixture()[name + "_err"][0]), Gn, seed, ont)
    return _reads[name]


def run_inputs(name, input_type, tmp):
    """the recorded run's input files in `tmp` -> dict(input, fasta, opts, tech, volume)"""
    from mecat_amd import workload as W
    K = fixture()
    codes, lens = read_set(name)
    fa = os.path.join(tmp, name + ".fasta")
    H.write_fasta(fa, codes, lens)
    inp = os.path.join(tmp, name + (".can", ".m4")[input_type])
    with open(inp, "wb") as f:
        f.write(lzma.decompress(K["%s_%s_input" % (name, ("can", "m4")[input_type])].tobytes()))
    return dict(input=inp, fasta=fa, opts=json.loads(str(K[name + "_opts"])), tech=TECH[name], input_type=input_type, volume=W.pack_volume(codes, lens))


def argv_of(run, out, threads=1):
    return ["-x", str(run["tech"]), "-i", str(run["input_type"]), "-t", str(threads)] + [x for kv in run["opts"].items() for x in kv] + [run["input"], run["fasta"], out]


def partition(run, tmp):
    """the m4 partition files of the run, written by the project's partition step with the program's arguments -> their paths in order"""
    o = run["opts"]
    assert run["input_type"] == 1
    subprocess.run([PARTITION, "-m", repr(float(o["-r"]) - 0.02), run["input"], o["-p"], o["-l"], "4"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
    return [l.split("\t")[0] for l in open(run["input"] + ".partition_files").read().splitlines()]


def group(recs, min_cov, min_size, tmp):
    """mecat_amd/cns/cns_groups.h on a partition file's records [n, 13] -> (the kept records in the driver's order, tmpl_begin, dropped [2])"""
    global _groups
    if _groups is None:
        so = os.path.join(tmp, "libcns_groups.so")
        subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-I" + os.path.join(H.ROOT, "mecat_amd", "cns"), "-I" + os.path.join(H.ROOT, "include"),
                        os.path.join(H.ROOT, "tests", "cns_groups_lib.cpp"), "-o", so], check=True)
        _groups = C.CDLL(so)
        _groups.cns_groups_make.restype = C.c_int64
        _groups.cns_groups_make.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    a = np.ascontiguousarray(recs, dtype=np.int32).copy()
    tb, dropped = np.zeros(len(a) + 1, np.int64), np.zeros(2, np.int64)
    nt = _groups.cns_groups_make(a.ctypes.data, len(a), int(min_cov), int(min_size), tb.ctypes.data, dropped.ctypes.data)
    tb = tb[: nt + 1].copy()
    return a[: tb[nt]], tb, dropped
