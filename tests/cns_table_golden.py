"""Readers of tests/golden/cns_table.npz (written by tests/golden/make_golden_cns_table.py from oracle/_ref/libref_cns_table.so: the
UNMODIFIED mecat2cns' consensus table), shared by test_cns_table_ref_cpu.py and test_gpu_cns_table.py.

Adversarial pairs: the 700 gap-normalised outputs of tests/golden/pushgaps.npz (strings read from that file) followed by the generated
pairs whose strings the fixture holds itself.  For pair i the fixture records soff, tmpl_len and what the reference's meap_add_one_aln
made of it on a fresh table: tmpl_len + 2 items {base, mat_cnt, ins_cnt, del_cnt}, the first and the last being the harness's guard items
(index -1 and tmpl_len of the reference's array)."""
import hashlib
import os

import numpy as np

import cns_table_ref as R
import helpers as H

_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = np.load(os.path.join(H.GOLDEN, "cns_table.npz"))
    return _cache["g"]


def planes_to_table(planes):
    """[4, n] uint8 (base, mat, ins, del planes: stored that way because they compress better) -> [n] TABLE_DTYPE"""
    return np.ascontiguousarray(planes.T).view(R.TABLE_DTYPE).reshape(-1)


def adversarial_pairs():
    """-> list of (q, s, soff, tmpl_len, table_with_guards [tmpl_len + 2] TABLE_DTYPE), q / s uint8 arrays; built once, read-only"""
    if "adv" not in _cache:
        g = golden()
        pg = np.load(os.path.join(H.GOLDEN, "pushgaps.npz"))
        assert hashlib.sha256(pg["qout"].tobytes() + pg["tout"].tobytes()).hexdigest() == str(g["adv_pushgaps_sha"])
        lens = np.concatenate([pg["lens"], g["adv_gen_lens"]]).astype(np.int64)
        q = np.concatenate([pg["qout"], g["adv_gen_q"]])
        s = np.concatenate([pg["tout"], g["adv_gen_s"]])
        soff, tl = g["adv_soff"], g["adv_tmpl_len"]
        assert len(lens) == len(soff) == len(tl)
        table = planes_to_table(g["adv_table"])
        cb = np.concatenate([[0], np.cumsum(lens)])
        tb = np.concatenate([[0], np.cumsum(tl.astype(np.int64) + 2)])
        assert tb[-1] == len(table)
        out = []
        for i in range(len(lens)):
            qi, si, ti = q[cb[i]: cb[i + 1]], s[cb[i]: cb[i + 1]], table[tb[i]: tb[i + 1]]
            for a in (qi, si, ti):
                a.flags.writeable = False
            out.append((qi, si, int(soff[i]), int(tl[i]), ti))
        _cache["adv"] = out
    return _cache["adv"]


def leading_run(q, s):
    """(the pair starts with a run of template gaps, that run holds a query base)"""
    sg = s == R.GAP
    if not sg[0]:
        return False, False
    end = int(np.argmin(sg)) if not sg.all() else len(s)
    return True, bool((q[:end] != R.GAP).any())


def template_of(s, soff, tmpl_len):
    """the letters of a template that the pair (., s, soff) aligns to: s without its gaps from soff on, 'A' elsewhere"""
    t = np.full(tmpl_len, ord("A"), dtype=np.uint8)
    b = s[s != R.GAP]
    t[soff: soff + len(b)] = b
    return t


# ---- fresh runs of the harness (build container only: need oracle/_ref/libref_cns_table.so) ------------------------------------------
def reference_tables(name, templates):
    """the reference's consensus_one_read_can_* on templates [0, templates) of a set of tests/golden/cns_accept.npz (same parameters, same
    candidates, read from that file) -> per template (meta [k, 3], sha of the strings, table [read_size] TABLE_DTYPE, ident uint8), or
    None for a template without candidates"""
    import ctypes as C
    import tempfile
    L = H.ref_cns_table()
    A = np.load(os.path.join(H.GOLDEN, "cns_accept.npz"))
    n, Lr, Gn, seed, ont, tech, mas = (int(x) for x in A[name + "_par"])
    err, ratio = (float(x) for x in A[name + "_ratio"])
    codes, lens = H.synth_reads(n, Lr, err, Gn, seed, ont)
    with tempfile.TemporaryDirectory(prefix="cnstab_") as d:
        fa = os.path.join(d, "r.fa")
        H.write_fasta(fa, codes, lens)
        assert L.refc_load_reads(fa.encode()) == n
    tb, cands = A[name + "_tmpl_begin"], A[name + "_cands"]
    sbuf = np.zeros(64 << 20, dtype=np.int8)
    out = []
    for t in range(templates):
        b, e = int(tb[t]), int(tb[t + 1])
        if e == b:
            out.append(None)
            continue
        cand = np.ascontiguousarray(cands[b:e]).copy()
        meta = np.zeros((128, 4), dtype=np.int32)
        table = np.zeros(int(lens.max()) + 8, dtype=R.TABLE_DTYPE)
        used, rs = C.c_long(), C.c_int()
        k = L.refc_consensus_can_table(tech, cand.ctypes.data, e - b, t, mas, ratio, meta.ctypes.data, sbuf.ctypes.data, len(sbuf), C.byref(used),
                                       table.ctypes.data, len(table), C.byref(rs))
        assert k >= 0, k
        assert rs.value == int(lens[t])
        table = table[: rs.value].copy()
        ident = np.zeros(rs.value, dtype=np.uint8)
        L.refc_identify_table(table.ctypes.data, rs.value, ident.ctypes.data)
        out.append((meta[:k, :3].copy(), hashlib.sha256(sbuf[: used.value].tobytes()).hexdigest(), table, ident))
    return out


def reference_add_one(q, s, soff, tmpl_len):
    """the reference's meap_add_one_aln on a fresh table -> [tmpl_len + 2] TABLE_DTYPE, guards first and last"""
    L = H.ref_cns_table()
    q, s = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(s, dtype=np.uint8)
    full = np.zeros(tmpl_len + 2, dtype=R.TABLE_DTYPE)
    full["base"] = ord("N")                                        # CnsTableItemCleaner's state
    inner = full[1: tmpl_len + 1].copy()
    guards = np.zeros(2, dtype=R.TABLE_DTYPE)
    rc = L.refc_add_one_aln(q.ctypes.data, s.ctypes.data, len(q), soff, inner.ctypes.data, tmpl_len, guards.ctypes.data)
    assert rc == 0, rc
    full[1: tmpl_len + 1] = inner
    full[0], full[-1] = guards[0], guards[1]
    return full


def reference_sweep():
    L = H.ref_cns_table()
    tri = np.ascontiguousarray(R.sweep_triples(), dtype=np.int32)
    out = np.zeros(len(tri), dtype=np.uint8)
    L.refc_identify_triples(tri.ctypes.data, len(tri), out.ctypes.data)
    return out
