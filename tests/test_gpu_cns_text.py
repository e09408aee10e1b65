"""The corrected reads' FASTA text on the device (mecat_amd/csrc/cns_text.hip; mhip_debug_cns_text, mhip_cns_correct_templates).  The
expected bytes are mhip_cns_format_reads' on the same records — the host formatting the text kernels replace, held to the reference's
records and text by test_gpu_cns_reads.py — and for the m4 walk what the unmodified consensus_one_read_m4_* recorded in
tests/golden/cns_cli.npz.  Everything goes through the C ABI."""
import hashlib
import os

import numpy as np
import pytest

import cns_plan_ref as PR
import cns_poa_cases as P
import helpers as H

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(H.GOLDEN, "cns_accept.npz"))
SIZES = (2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 49000)
INT_MAX = 2147483647


@pytest.fixture(scope="module")
def ctx():
    import mecat_amd.hip as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def letters():
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(5).integers(0, 4, 70000)]


def number(rng, digits):
    """a value with that many decimal digits"""
    lo, hi = (0 if digits == 1 else 10 ** (digits - 1)), min(10 ** digits - 1, INT_MAX)
    return int(rng.integers(lo, hi + 1))


def record(M, rng, size, seq_begin, pos, dst_residue, t=None):
    """a record whose letters land at text position = dst_residue (mod 16) when its text begins at `pos`: the three free numbers'
    digit counts (t: 3 .. 30 in all; the smallest that fits when not given) choose the header's length"""
    ds = len(str(size))
    if t is None:
        t = 3 + (dst_residue - (pos + 5 + ds + 3)) % 16
    d1 = min(10, t - 2)
    d2 = min(10, t - d1 - 1)
    d3 = t - d1 - d2
    assert 1 <= d3 <= 10
    r = np.zeros(1, M.READ_DTYPE)[0]
    r["read_id"], r["range_beg"], r["range_end"], r["size"], r["seq_begin"] = number(rng, d1), number(rng, d2), number(rng, d3), size, seq_begin
    hl = 5 + ds + t
    assert (pos + hl) % 16 == dst_residue
    return r, hl + size + 1


def both(ctx, reads, seq):
    import mecat_amd.hip as M
    want = M.cns_format_reads(reads, seq)
    got = M.debug_cns_text(ctx, reads, seq)
    assert len(got) == len(want)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError("first difference at byte %d of %d: %r != %r" % (i, len(want), got[max(0, i - 20): i + 20], want[max(0, i - 20): i + 20]))
    return want


@pytest.mark.parametrize("size", SIZES)
def test_sizes_at_every_alignment(ctx, letters, size):
    """one size, the source at each of the 16 residues mod 16 and the destination at each of the 16: 256 records in one call"""
    import mecat_amd.hip as M
    rng = np.random.default_rng(size)
    recs, pos, seen = [], 0, set()
    for src in range(16):
        for dst in range(16):
            begin = 16 * int(rng.integers(0, (len(letters) - size - 16) // 16)) + src
            r, n = record(M, rng, size, begin, pos, dst)
            recs.append(r)
            seen.add((begin % 16, (pos + n - size - 1) % 16))
            pos += n
    assert len(seen) == 256
    text = both(ctx, np.array(recs, M.READ_DTYPE), letters)
    assert len(text) == pos and text.count(b">") == 256


def test_header_lengths(ctx, letters):
    """every header length a record over these letters can have: 9 (four one-digit numbers) to 40 (three ten-digit numbers and a
    five-digit size; the lengths up to 45 need a size of ten digits: test_cns_text_ref_cpu.py), and the numbers at their ends"""
    import mecat_amd.hip as M
    rng = np.random.default_rng(1)
    recs, pos = [], 0
    for ds in range(1, 6):
        for t in range(3, 31):
            size = min(number(rng, ds), 60000)
            r, n = record(M, rng, size, int(rng.integers(0, 1000)), pos, (pos + 5 + ds + t) % 16, t)
            assert n == 5 + ds + t + size + 1
            recs.append(r)
            pos += n
    for ids in ((0, 0, 0), (INT_MAX, INT_MAX, INT_MAX), (9, 10, 99), (1000000000, 999999999, 0)):
        for size in (0, 2, 9, 10, 60000):
            r = np.zeros(1, M.READ_DTYPE)[0]
            r["read_id"], r["range_beg"], r["range_end"], r["size"], r["seq_begin"] = ids + (size, 3)
            recs.append(r)
    reads = np.array(recs, M.READ_DTYPE)
    text = both(ctx, reads, letters)
    assert {len(l) + 1 for l in text.split(b"\n") if l.startswith(b">")} == set(range(9, 41))
    assert text.startswith(b">%d_%d_%d_%d\n" % tuple(int(reads[0][k]) for k in ("read_id", "range_beg", "range_end", "size")))


def test_cut_target(ctx, letters):
    """a 60 001-letter target cut into its two overlapping records (csrc/cns_reads.h's rule), both pointing into the one stored stretch"""
    import ctypes as C
    import mecat_amd.hip as M
    L = P.host_lib()
    L.cns_reads_host_blocks.restype = C.c_int64
    L.cns_reads_host_blocks.argtypes = [C.c_int64]
    L.cns_reads_host_block.argtypes = [C.c_int64] * 4 + [C.c_void_p]
    size, beg, end, at = 60001, 120, 59000, 5
    assert L.cns_reads_host_blocks(size) == 2
    reads = np.zeros(2, M.READ_DTYPE)
    for k in range(2):
        o = (C.c_int64 * 4)()
        L.cns_reads_host_block(size, k, beg, end, o)
        reads[k] = (77, o[2], o[3], o[1] - o[0], at + o[0], 0, 0)
    assert reads["size"].tolist() == [49000, 21001] and reads["seq_begin"].tolist() == [at, at + 39000]
    text = both(ctx, reads, letters)
    lines = text.split(b"\n")
    assert lines[1][39000:] == lines[3][:10000] and lines[1] + lines[3][10000:] == letters[at: at + size].tobytes()


def test_edge_counts(ctx, letters):
    import mecat_amd.hip as M
    assert M.debug_cns_text(ctx, np.zeros(0, M.READ_DTYPE), letters) == b""
    assert M.debug_cns_text(ctx, np.zeros(0, M.READ_DTYPE), np.zeros(0, np.uint8)) == b""
    rng = np.random.default_rng(2)
    reads = np.zeros(1025, M.READ_DTYPE)          # crosses the scan's tile of 1 024
    reads["read_id"] = np.arange(1025)
    reads["range_end"] = rng.integers(0, 100000, 1025)
    reads["size"] = rng.integers(2, 40, 1025)
    reads["seq_begin"] = rng.integers(0, 60000, 1025)
    text = both(ctx, reads, letters)
    assert text.count(b"\n") == 2 * 1025


def test_refusal_launches_nothing(ctx, letters):
    import mecat_amd.hip as M
    reads = np.zeros(3, M.READ_DTYPE)
    reads["size"] = 100
    reads["seq_begin"] = [0, len(letters) - 99, 5]          # the second leaves seq by one letter
    ctx.set_profiling(True)
    ctx.reset_stats()
    try:
        for bad in (reads, reads[1:2]):
            with pytest.raises(M.MhipError) as e:
                M.debug_cns_text(ctx, bad, letters)
            assert "leaves the letters" in str(e.value)
        neg = reads[:1].copy()
        neg["range_beg"] = -1
        with pytest.raises(M.MhipError) as e:
            M.debug_cns_text(ctx, neg, letters)
        assert "negative" in str(e.value)
        assert not [k for k in ctx.kernel_stats() if k.startswith("cns_text")]
        M.debug_cns_text(ctx, reads[:1], letters)
        assert sorted(k for k in ctx.kernel_stats() if k.startswith("cns_text")) == ["cns_text_scan", "cns_text_size", "cns_text_write"]
    finally:
        ctx.set_profiling(False)


# ---- the whole call on the accept fixture's two sets ----------------------------------------------------------------------------------

_sets = {}


def golden_set(name, n):
    if (name, n) not in _sets:
        from mecat_amd import workload as W
        nr, L, Gn, seed, ont, tech, mas = (int(x) for x in G[name + "_par"])
        err, ratio = (float(x) for x in G[name + "_ratio"])
        codes, lens = W.synth_reads(nr, L, err, Gn, seed, ont)
        pac, offs, nb = W.pack_volume(codes, lens)
        tb = G[name + "_tmpl_begin"][: n + 1].copy()
        _sets[name, n] = dict(pac=pac, offs=offs, nb=nb, lens=lens, tb=tb, cands=G[name + "_cands"][: tb[n]].copy(), tech=tech, mas=mas, ratio=ratio)
    return _sets[name, n]


def correct(ctx, g, want, params, input_type=0):
    import mecat_amd.hip as M
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], 0)
    try:
        return M.cns_correct_templates(ctx, vol, g["cands"], g["tb"], g["tech"], g["mas"], g["ratio"], want, *params, input_type=input_type, threads=16)
    finally:
        vol.free()


def same(x, y):
    """two outputs in cns_accept_templates_reads' shape, field for field"""
    for p, q in zip(x, y):
        if isinstance(p, dict) or isinstance(q, dict):
            assert isinstance(p, dict) and isinstance(q, dict) and sorted(p) == sorted(q) and all(np.asarray(p[k]).tobytes() == np.asarray(q[k]).tobytes() for k in p)
        elif p is None or q is None:
            assert p is None and q is None
        else:
            assert np.asarray(p).tobytes() == np.asarray(q).tobytes()


@pytest.mark.parametrize("name,n,params", [("pacbio", 48, (4, 3000)), ("nanopore", 32, None)])
def test_whole_call(ctx, monkeypatch, name, n, params):
    import mecat_amd.hip as M
    S, TB, PL, PC, PO, RD, TX = M.CNS_WANT_STRINGS, M.CNS_WANT_TABLE, M.CNS_WANT_PLAN, M.CNS_WANT_PIECES, M.CNS_WANT_POA, M.CNS_WANT_READS, M.CNS_WANT_TEXT
    g = golden_set(name, n)
    params = params or PR.DEFAULTS[g["tech"]]
    # TEXT | READS: the text is the host formatting of the same call's records
    out, text, _, null = correct(ctx, g, TX | RD, params)
    rd = out[7]
    print(name, n, "records", len(rd["reads"]), "letters", len(rd["seq"]), "text", len(text))
    assert len(rd["reads"]) >= 3 and text == M.cns_format_reads(rd["reads"], rd["seq"])
    # TEXT alone: the same text; the accepted records and nothing else
    out1, text1, _, null1 = correct(ctx, g, TX, params)
    assert text1 == text and out1[0].tobytes() == out[0].tobytes() and len(out1[0]) > 0 and np.all(out1[0]["str_offset"] == -1)
    assert [k for k, v in null1.items() if not v] == ["accepted", "text"] and out1[2] == out[2]
    # at least 3 slices: both scratch sets are used again
    monkeypatch.setenv("MECAT_CNS_SLICE_JOBS", str(max(1, out[2] // 4)))
    many, textm, _, _ = correct(ctx, g, TX, params)
    monkeypatch.delenv("MECAT_CNS_SLICE_JOBS")
    assert textm == text and many[0].tobytes() == out[0].tobytes()
    # input_type 0 without TEXT is mhip_cns_accept_templates_reads, field for field
    vol = M.Volume(ctx, g["pac"], g["offs"], g["nb"], 0)
    try:
        for w in (S | TB | PL | PC | PO | RD, RD, PL | PO, S):
            ref = M.cns_accept_templates_reads(ctx, vol, g["cands"].copy(), g["tb"], g["tech"], g["mas"], g["ratio"], w, *params, threads=16)
            ref = tuple(np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in ref)
            got, t, _, _ = M.cns_correct_templates(ctx, vol, g["cands"], g["tb"], g["tech"], g["mas"], g["ratio"], w, *params, threads=16)
            assert t is None and got[2] == ref[2]
            same(got[:2] + got[3:], ref[:2] + ref[3:])
        # the existing entry points keep refusing the bit
        with pytest.raises(M.MhipError):
            M.cns_accept_templates_reads(ctx, vol, g["cands"].copy(), g["tb"], g["tech"], g["mas"], g["ratio"], RD | TX, *params, threads=16)
    finally:
        vol.free()


# ---- the m4 walk against the unmodified consensus_one_read_m4_* ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pacbio", "nanopore"])
def test_m4_walk(ctx, tmp_path, name):
    """mhip_cns_correct_templates(input_type = 1) on the recorded m4 partitions: per template the acceptances (order, coordinates, string
    hashes) and the cns_results of the reference, the templates handed over the way the driver does (cns_cli_cases.py)"""
    import mecat_amd.hip as M
    import cns_cli_cases as CC
    K = CC.fixture()
    key = name + "_m4"
    run = CC.run_inputs(name, 1, str(tmp_path))
    o = run["opts"]
    tech, mas, ratio, min_cov, min_size = run["tech"], int(o["-a"]), float(o["-r"]), int(o["-c"]), int(o["-l"])
    parts = CC.partition(run, str(tmp_path))
    assert len(parts) >= 3
    pac, offs, nb = run["volume"]
    vol = M.Volume(ctx, pac, offs, nb, 0)
    counts, meta, sha, sids = K[key + "_walk_counts"], CC.table(key + "_walk_meta", 3), K[key + "_walk_sha"], K[key + "_walk_sid"]
    results, result_sha = K[key + "_walk_results"], K[key + "_walk_result_sha"]
    k = m0 = r0 = 0
    try:
        for path in parts:
            recs, tb, dropped = CC.group(np.fromfile(path, dtype=np.int32).reshape(-1, 13), min_cov, min_size, str(tmp_path))
            nt = len(tb) - 1
            out, text, cands, _ = M.cns_correct_templates(ctx, vol, recs, tb, tech, mas, ratio, M.CNS_WANT_STRINGS | M.CNS_WANT_READS, min_cov, min_size, input_type=1, threads=16)
            acc, strings, rd = out[0], out[1], out[7]
            assert text is None and out[2] == int(np.minimum(np.diff(tb), CC.MAX_ADDED[name]).sum())
            for t in range(nt):
                nrec, looked, aligned, refused, nacc, nres = (int(x) for x in counts[k])
                assert int(cands[tb[t], 7]) == int(sids[k]) and tb[t + 1] - tb[t] == nrec, (path, t)
                a = acc[acc["template_index"] == t]
                assert [(int(x["soff"]), int(x["send"]), int(x["aln_size"])) for x in a] == [tuple(int(v) for v in m) for m in meta[m0: m0 + nacc]], (path, t)
                h = hashlib.sha256()
                for x in a:
                    h.update(strings[int(x["str_offset"]): int(x["str_offset"]) + 2 * (int(x["aln_size"]) + 1)].tobytes())
                assert h.hexdigest() == str(sha[k]), (path, t)
                mine = rd["reads"][rd["read_begin"][t]: rd["read_begin"][t + 1]]
                assert [(int(x["read_id"]), int(x["range_beg"]), int(x["range_end"]), int(x["size"])) for x in mine] == [tuple(int(v) for v in r) for r in results[r0: r0 + nres]], (path, t)
                assert [hashlib.sha256(rd["seq"][int(x["seq_begin"]): int(x["seq_begin"]) + int(x["size"])].tobytes()).hexdigest() for x in mine] == [str(s) for s in result_sha[r0: r0 + nres]]
                k, m0, r0 = k + 1, m0 + nacc, r0 + nres
    finally:
        vol.free()
    assert k == len(counts) and m0 == len(meta) and r0 == len(results) and k >= 100
