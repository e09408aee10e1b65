"""Inputs and fixture access shared by the tests of mecat2ref's extension stage (tests/golden/ref_ext.npz, made by
tests/golden/make_golden_ref_ext.py from the unmodified reference; reference, reads and candidate lists are ref_cand.npz's)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import helpers as H
import ref_cand_cases as RC
import ref_cand_ref as R

FIXTURE = os.path.join(H.GOLDEN, "ref_ext.npz")
CAND_FIELDS = ("read", "chain", "loc1", "loc2", "score")
RES_FIELDS = ("ok", "qb", "qe", "qs", "sb", "se", "cols")
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def pack_reads(read_list):
    """mecat_amd/host/ref_reads.cpp's twin: reads as letters -> (pac, nplane, offs int32[n, 2], num_bases).  pac holds the code the tool's
    extension gives a letter (get_dna_encode_table: lower-case a, c, g, t are 0..3 too, every other letter 0), nplane is 3 at every letter
    that is not an upper-case A, C, G or T; the volume layout (first base in the two top bits of a byte, one pad base behind every read)"""
    import ref_ext_ref as X
    n = len(read_list)
    offs = np.zeros((n, 2), dtype=np.int32)
    tot = sum(len(r) + 1 for r in read_list)
    codes = np.zeros(tot + 4, dtype=np.uint8)
    nn = np.zeros(tot + 4, dtype=np.uint8)
    upper = np.zeros(256, dtype=bool)
    upper[LETTERS] = True
    p = 0
    for i, r in enumerate(read_list):
        r = np.asarray(r, dtype=np.uint8)
        offs[i] = (p, len(r))
        codes[p: p + len(r)] = X.ENCODE[r]
        nn[p: p + len(r)] = np.where(upper[r], 0, 3)
        p += len(r) + 1

    def pk(a):
        a = a[: (tot + 3) // 4 * 4].reshape(-1, 4)
        return (a[:, 0] << 6 | a[:, 1] << 4 | a[:, 2] << 2 | a[:, 3]).astype(np.uint8)
    return pk(codes), pk(nn), offs, tot


def ref_codes(ref_fasta):
    """the concatenated reference as the extension reads it: codes, every letter that is not A, C, G, T as 0"""
    import ref_ext_ref as X
    let, _ = R.read_reference(ref_fasta)
    return X.ENCODE[R.upper(let)], R.upper(let)


_fx = None


def fixture():
    """ref_ext.npz + ref_cand.npz's reads and reference: cands int64[n, 5] (CAND_FIELDS), res int64[n, 7] (RES_FIELDS), crc uint32[n, 2]
    (ok results), source (per candidate: 1 / 2 = the recorded PacBio -n 10 list of that round, 0 = hand-made), stored / stored_offs /
    stored_words (the subset whose columns are kept)"""
    global _fx
    if _fx is None:
        z = np.load(FIXTURE)
        _fx = {k: z[k] for k in z.files}
        base = RC.fixture()
        _fx["read_list"] = base["read_list"]
        _fx["ref_fasta"] = base["ref_fasta"].tobytes()
        _fx["ref_codes"], _fx["ref_letters"] = ref_codes(_fx["ref_fasta"])
    return _fx


def tables(cands, nreads):
    """cands int64[m, 5] in any order -> (table [nreads, maxc] REF_CAND_DTYPE, counts, slot_of int[m]): each read's candidates in the
    order given, maxc = the longest list"""
    from mecat_amd import hip
    cands = np.asarray(cands, dtype=np.int64).reshape(-1, 5)
    cnt = np.zeros(nreads, dtype=np.int32)
    maxc = max(1, int(np.bincount(cands[:, 0], minlength=nreads).max())) if len(cands) else 1
    tab = np.zeros((nreads, maxc), dtype=hip.REF_CAND_DTYPE)
    slot = np.zeros(len(cands), dtype=np.int64)
    for i, (rd, ch, l1, l2, sc) in enumerate(cands):
        k = cnt[rd]
        tab[rd, k]["loc1"], tab[rd, k]["loc2"], tab[rd, k]["chain"], tab[rd, k]["score"] = l1, l2, ch, sc
        slot[i] = rd * maxc + k
        cnt[rd] += 1
    return tab, cnt, slot


# ----------------------------------------------------------------------------- mecat_amd/host/ref_results.cpp + ref_reads.cpp through tests/ref_results_lib.cpp
_rl = None


def results_lib():
    global _rl
    if _rl is None:
        libdir = os.path.join(H.ROOT, "mecat_amd", "lib")
        so = os.path.join(tempfile.mkdtemp(prefix="refresults_"), "libref_results.so")
        subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-I" + os.path.join(H.ROOT, "include"), os.path.join(H.ROOT, "tests", "ref_results_lib.cpp"),
                        "-L" + libdir, "-lmecat_hip", "-Wl,-rpath," + libdir, "-o", so], check=True)
        L = C.CDLL(so)
        L.rr_pack.restype = C.c_int64
        L.rr_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rr_strings.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rr_record.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int]
        L.rr_align_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _rl = L
    return _rl


def lib_pack_reads(read_list):
    """ref_reads_pack -> (pac, nplane, offs, num_bases)"""
    L = results_lib()
    text = np.concatenate([np.asarray(r, dtype=np.uint8) for r in read_list] + [np.zeros(1, dtype=np.uint8)])
    lens = np.array([len(r) for r in read_list], dtype=np.int32)
    tot = int(lens.sum()) + len(lens)
    pac, npl = np.zeros((tot + 3) // 4, dtype=np.uint8), np.zeros((tot + 3) // 4, dtype=np.uint8)
    offs = np.zeros((len(lens), 2), dtype=np.int32)
    assert L.rr_pack(text.ctypes.data, lens.ctypes.data, len(lens), pac.ctypes.data, npl.ctypes.data, offs.ctypes.data) == tot
    return pac, npl, offs, tot


def lib_strings(res_row, words, reads_pac, reads_nplane, read_off, ref_pac):
    """ref_result_strings on one mhip_ref_result (a REF_RESULT_DTYPE record) -> (qmap, smap) bytes, or None when the walk does not add up"""
    L = results_lib()
    cols = int(res_row["cols"])
    q, s = C.create_string_buffer(cols + 1), C.create_string_buffer(cols + 1)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    rec = np.ascontiguousarray(res_row).reshape(1)
    ok = L.rr_strings(rec.ctypes.data, words.ctypes.data, reads_pac.ctypes.data, reads_nplane.ctypes.data, int(read_off), ref_pac.ctypes.data, q, s)
    return (q.raw[:cols], s.raw[:cols]) if ok else None


def lib_record(read_id, res_row, qmap, smap):
    L = results_lib()
    buf = C.create_string_buffer(2 * len(qmap) + 256)
    rec = np.ascontiguousarray(res_row).reshape(1)
    n = L.rr_record(read_id, rec.ctypes.data, qmap, smap, buf, len(buf))
    return buf.raw[:n]


def lib_align_info(res_row, idx):
    """-> (qoff, qend, parent_id, id, prev_id, next_id, valid, qdir, soff, send)"""
    out = np.zeros(10, dtype=np.int64)
    rec = np.ascontiguousarray(res_row).reshape(1)
    results_lib().rr_align_info(rec.ctypes.data, idx, out.ctypes.data)
    return tuple(int(x) for x in out)
