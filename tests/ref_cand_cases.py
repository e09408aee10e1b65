"""Inputs and fixture access shared by the tests of mecat2ref's candidate stage (tests/golden/ref_cand.npz, made by
tests/golden/make_golden_ref_cand.py from the unmodified reference)."""
import ctypes as C
import os

import numpy as np

import helpers as H

FIXTURE = os.path.join(H.GOLDEN, "ref_cand.npz")
FIELDS = ("loc1", "loc2", "left1", "left2", "right1", "right2", "score", "num1", "num2", "chain")
RUNS = [(tech, n) for n in (10, 3) for tech in (0, 1)]          # (technology, -n) of the recorded runs
CUTOFF = {0: 0.25, 1: 0.25}          # the tool names 0.1 for nanopore and never assigns it: both technologies run at 0.25
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def genome(n, seed):
    """libsynth's genome -> codes uint8[n]"""
    lib = H.synth_lib()
    lib.synth_genome.argtypes = [C.c_void_p, C.c_int64, C.c_uint64]
    g = np.empty(n, dtype=np.uint8)
    lib.synth_genome(g.ctypes.data, n, seed)
    return g


def one_read(g, idx, L, err, seed, ont=0):
    """libsynth's read `idx` of length about L at error rate err from a random place and strand of g -> codes"""
    lib = H.synth_lib()
    lib.synth_rates.argtypes = [C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.synth_one_read.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_void_p, C.c_int]
    pd, ps, pi = C.c_double(), C.c_double(), C.c_double()
    lib.synth_rates(err, ont, C.byref(pd), C.byref(ps), C.byref(pi))
    g = np.ascontiguousarray(g, dtype=np.uint8)
    cap = int(min(L, len(g)) * 1.25) + 64
    out = np.empty(cap, dtype=np.uint8)
    n = lib.synth_one_read(g.ctypes.data, len(g), idx, L, pd.value, ps.value, pi.value, seed, out.ctypes.data, cap)
    return out[:n].copy()


def letters(codes):
    return LETTERS[np.asarray(codes, dtype=np.uint8)]


def fasta_bytes(names, seqs, width=0):
    """records as FASTA text; width 0 = one line per sequence"""
    out = []
    for name, s in zip(names, seqs):
        s = bytes(np.asarray(s, dtype=np.uint8))
        out.append(b">" + name + b"\n")
        if width:
            out += [s[i: i + width] + b"\n" for i in range(0, len(s), width)]
        else:
            out.append(s + b"\n")
    return b"".join(out)


def parse_reads(text):
    """a FASTA file with one line per sequence -> [letters uint8[]]"""
    lines = bytes(text).split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1
    assert all(lines[i][:1] == b">" for i in range(0, len(lines) - 1, 2))
    return [np.frombuffer(lines[i], dtype=np.uint8) for i in range(1, len(lines), 2)]


_fx = None


def fixture():
    global _fx
    if _fx is None:
        z = np.load(FIXTURE)
        _fx = {k: z[k] for k in z.files}
        _fx["read_list"] = parse_reads(_fx["reads_fasta"].tobytes())
    return _fx


def recorded(fx, tech, n, rnd):
    """-> per read the recorded candidate list as int64[count, 10] (FIELDS order)"""
    key = "t%d_n%d_r%d" % (tech, n, rnd)
    cnt = fx[key + "_counts"]
    tab = fx[key + "_cands"].astype(np.int64).reshape(-1, len(FIELDS))
    ends = np.cumsum(cnt)
    return [tab[e - c: e] for c, e in zip(cnt, ends)]


def pack_reads(read_list):
    """reads as letters -> (pac, nplane, offs int32[n, 2], num_bases): the volume layout (first base in the two top bits of a byte, one
    pad base behind every read), the N plane 3 at every letter that is not an upper-case A, C, G or T (mecat2ref does not upper-case
    reads) and code 0 in pac there"""
    n = len(read_list)
    offs = np.zeros((n, 2), dtype=np.int32)
    tot = sum(len(r) + 1 for r in read_list)
    codes = np.zeros(tot + 4, dtype=np.uint8)
    nn = np.zeros(tot + 4, dtype=np.uint8)
    lut = np.full(256, 4, dtype=np.uint8)
    lut[LETTERS] = np.arange(4)
    p = 0
    for i, r in enumerate(read_list):
        c = lut[r]
        offs[i] = (p, len(r))
        codes[p: p + len(r)] = np.where(c < 4, c, 0)
        nn[p: p + len(r)] = np.where(c < 4, 0, 3)
        p += len(r) + 1

    def pk(a):
        a = a[: (tot + 3) // 4 * 4].reshape(-1, 4)
        return (a[:, 0] << 6 | a[:, 1] << 4 | a[:, 2] << 2 | a[:, 3]).astype(np.uint8)
    return pk(codes), pk(nn), offs, tot


# ----------------------------------------------------------------------------- mecat_amd/host/ref_genome.cpp through tests/ref_genome_lib.cpp
_rg = None


def ref_genome_lib():
    global _rg
    if _rg is None:
        import subprocess
        import tempfile
        libdir = os.path.join(H.ROOT, "mecat_amd", "lib")
        so = os.path.join(tempfile.mkdtemp(prefix="refgenome_"), "libref_genome.so")
        subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-I" + os.path.join(H.ROOT, "include"), os.path.join(H.ROOT, "tests", "ref_genome_lib.cpp"),
                        "-L" + libdir, "-lmecat_hip", "-Wl,-rpath," + libdir, "-o", so], check=True)
        L = C.CDLL(so)
        L.rg_parse.restype = C.c_void_p
        L.rg_parse.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int]
        L.rg_free.argtypes = [C.c_void_p]
        L.rg_sizes.argtypes = [C.c_void_p, C.c_void_p]
        L.rg_copy.argtypes = [C.c_void_p] * 5
        L.rg_upload.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        _rg = L
    return _rg


class RefGenome:
    """ref_genome_parse on the file's bytes: pac, nplane, reads int32[n, 2], chrindex bytes, num_bases; .h for rg_upload"""

    def __init__(self, text):
        L = ref_genome_lib()
        err = C.create_string_buffer(256)
        self.h = L.rg_parse(bytes(text), len(text), err, 256)
        if not self.h:
            raise ValueError(err.value.decode())
        sz = np.zeros(4, dtype=np.int64)
        L.rg_sizes(self.h, sz.ctypes.data)
        self.num_bases, nreads, nchr, self.num_chroms = (int(x) for x in sz)
        nb = (self.num_bases + 3) // 4
        self.pac, self.nplane = np.zeros(nb, dtype=np.uint8), np.zeros(nb, dtype=np.uint8)
        self.reads = np.zeros((nreads, 2), dtype=np.int32)
        buf = C.create_string_buffer(nchr + 1)
        L.rg_copy(self.h, self.pac.ctypes.data, self.nplane.ctypes.data, self.reads.ctypes.data, buf)
        self.chrindex = buf.raw[:nchr]

    def upload(self, ctx):
        """ref_genome_upload -> (Volume, Index) of mecat_amd.hip around the handles it made"""
        from mecat_amd import hip
        v, i = C.c_void_p(), C.c_void_p()
        if ref_genome_lib().rg_upload(ctx.h, self.h, C.byref(v), C.byref(i)):
            raise hip.MhipError(hip.lib().mhip_last_error().decode())
        vol = hip.Volume.__new__(hip.Volume)
        vol.h, vol.offs, vol.num_reads, vol.num_bases, vol.start_read_id = v, self.reads, len(self.reads), self.num_bases, 0
        idx = hip.Index.__new__(hip.Index)
        idx.h, idx.ctx = i, ctx
        return vol, idx

    def free(self):
        if self.h:
            ref_genome_lib().rg_free(self.h)
            self.h = None
