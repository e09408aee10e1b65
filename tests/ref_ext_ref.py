"""Plain restatement of mecat2ref's extension of one candidate, with the aligned strings: extract_sequences
(mecat2ref/mecat2ref_aux.cpp:85-121) + DiffAligner::go (common/diff_gapalign.cpp:294-349) with dw_in_one_direction (:221-292),
retrieve_next_aln_block and trim_mismatch_end (common/gapalign.cpp:9-68).  Python does the chaining; the per-block Align and its two
strings are liboracle's orc_align.  tests/test_ref_ext_cpu.py pins it to what the unmodified tool recorded (tests/golden/ref_ext.npz)."""
import ctypes as C

import numpy as np

import helpers as H

SEG = 500          # DiffAlignParameters::segment_size
GAP = 4
MIN_COLS = 1000          # extend_candidate's min_aln_size

# get_dna_encode_table followed by `if (c > 3) c = 0` (common/defs.cpp:3-33, mecat2ref_aux.cpp:107-119)
ENCODE = np.zeros(256, dtype=np.uint8)
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    for _ch in _pair:
        ENCODE[_ch] = _i
_COMP_UPPER = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP_UPPER[_a] = _b


def strand_letters(read, chain):
    """reference_mapping's strands (mecat2ref_impl_large.cpp:374-408): the reverse one is the read reversed with only upper-case A, C, G,
    T complemented"""
    read = np.asarray(read, dtype=np.uint8)
    return _COMP_UPPER[read[::-1]] if chain else read


def window(ref_size, read_len, loc1, loc2):
    """extract_sequences' arithmetic -> (ref_start, read_start, left_ref_size, right_ref_size)"""
    ref_start, read_start = int(loc1) - 1, int(loc2)
    L = min(read_start, ref_start)
    R = min(read_len - read_start, ref_size - ref_start)
    return ref_start, read_start, min(ref_start, int(L * 1.2)), min(ref_size - ref_start, int(R * 1.2))


_al = None


def _aligner():
    global _al
    if _al is None:
        _al = H.orc().orc_aligner_new()
    return _al


def one_direction(q, t, right):
    """dw_in_one_direction over the direction's sequences IN EXTENSION ORDER (codes) -> (query string, target string, facts): the
    strings in extension order over 0..3 and GAP; facts = dict(blocks, sized_last, fallback, tail_rows)"""
    q = np.ascontiguousarray(q, dtype=np.uint8)
    t = np.ascontiguousarray(t, dtype=np.uint8)
    L = H.orc()
    res = np.zeros(6, dtype=np.int32)
    qa, ta = np.zeros(4096, dtype=np.uint8), np.zeros(4096, dtype=np.uint8)
    qidx = tidx = 0
    qs, ts = [], []
    facts = dict(blocks=0, sized_last=0, fallback=0, tail_rows=0)
    while True:
        qleft, tleft = len(q) - qidx, len(t) - tidx
        if qleft < SEG + 100 or tleft < SEG + 100:
            qblk, tblk, last = min(qleft, int(tleft + tleft * 0.2)), min(tleft, int(qleft + qleft * 0.2)), True
        else:
            qblk, tblk, last = SEG, SEG, False
        bq, bt = q[qidx: qidx + qblk], t[tidx: tidx + tblk]
        if not right:          # orc_align reads a left block from its last element backwards
            bq, bt = np.ascontiguousarray(bq[::-1]), np.ascontiguousarray(bt[::-1])
        reached = L.orc_align(_aligner(), bq.ctypes.data, qblk, bt.ctypes.data, tblk, int(0.3 * max(qblk, tblk)), 400, int(bool(right)), res.ctypes.data,
                              qa.ctypes.data, ta.ctypes.data)
        facts["blocks"] += 1
        size, qe, te = int(res[0]), int(res[3]), int(res[5])
        # trim_mismatch_end(.., 4, ..)
        m = qcnt = tcnt = acnt = 0
        k = size - 1
        while k >= 0 and m < 4:
            acnt += 1
            qcnt += qa[k] != GAP
            tcnt += ta[k] != GAP
            m = m + 1 if qa[k] == ta[k] else 0
            k -= 1
        if not (m == 4 and k > 0):
            break
        facts["sized_last"] |= int(last and (qblk < qleft or tblk < tleft))
        facts["fallback"] += int(not reached)
        facts["tail_rows"] = max(facts["tail_rows"], int((qa[size - acnt: size] != ta[size - acnt: size]).sum()))
        full_map = qblk - qe <= 20 or tblk - te <= 20
        if last or not full_map:
            qcnt, tcnt, acnt = qcnt - 4, tcnt - 4, acnt - 4
        qs.append(qa[: size - acnt].copy())
        ts.append(ta[: size - acnt].copy())
        if last or not full_map:
            break
        qidx += qe - int(qcnt)
        tidx += te - int(tcnt)
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.uint8)
    return cat(qs), cat(ts), facts


def extend(ref_codes, read_letters, chain, loc1, loc2):
    """extend_candidate for one candidate -> dict(ok, qb, qe, qs, sb, se, cols, qmap, smap (bytes over b"ACGT-"), left, right (facts))
    ref_codes: the concatenated reference as codes (every letter that is not A, C, G, T is 0)"""
    ref_codes = np.asarray(ref_codes, dtype=np.uint8)
    q = ENCODE[strand_letters(read_letters, chain)]
    ref_start, read_start, left, right = window(len(ref_codes), len(q), loc1, loc2)
    lq, lt, lf = one_direction(q[:read_start][::-1], ref_codes[ref_start - left: ref_start][::-1], False)
    rq, rt, rf = one_direction(q[read_start:], ref_codes[ref_start: ref_start + right], True)
    qm = np.concatenate([lq[::-1], rq])
    sm = np.concatenate([lt[::-1], rt])
    dt = np.frombuffer(b"ACGT-", dtype=np.uint8)
    return dict(ok=int(len(qm) >= MIN_COLS), qb=read_start - int((lq != GAP).sum()), qe=read_start + int((rq != GAP).sum()), qs=len(q),
                sb=ref_start - int((lt != GAP).sum()), se=ref_start + int((rt != GAP).sum()), cols=len(qm), qmap=dt[qm].tobytes(), smap=dt[sm].tobytes(),
                left=lf, right=rf, lcols=len(lq), rcols=len(rq))


def columns_of(qmap, smap):
    """the two strings -> the 2-bit columns (0 = both bases, 1 = target base only, 2 = query base only), 16 per uint32 from the low end"""
    a, b = np.frombuffer(qmap, dtype=np.uint8), np.frombuffer(smap, dtype=np.uint8)
    assert len(a) == len(b) and not ((a == 45) & (b == 45)).any() and ((a == b) | (a == 45) | (b == 45)).all(), "a mismatch column"
    op = np.where(a == 45, 1, np.where(b == 45, 2, 0)).astype(np.uint64)
    op = np.concatenate([op, np.zeros(-len(op) % 16, dtype=np.uint64)]).reshape(-1, 16)
    return (op << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


def strings_of(words, cols, q_strand_codes, ref_codes, qb, sb):
    """columns + codes + start coordinates -> (qmap, smap, qe, se): the forward walk mecat_amd/host/ref_results.cpp does"""
    op = ((np.repeat(np.asarray(words, dtype=np.uint32), 16) >> np.tile(2 * np.arange(16, dtype=np.uint32), len(words))) & 3)[:cols]
    assert not (op == 3).any()
    qi = qb + np.cumsum(op != 1) - 1
    si = sb + np.cumsum(op != 2) - 1
    dt = np.frombuffer(b"ACGT", dtype=np.uint8)
    qm = np.where(op != 1, dt[np.asarray(q_strand_codes)[np.clip(qi, 0, None)]], 45).astype(np.uint8)
    sm = np.where(op != 2, dt[np.asarray(ref_codes)[np.clip(si, 0, None)]], 45).astype(np.uint8)
    return qm.tobytes(), sm.tobytes(), qb + int((op != 1).sum()), sb + int((op != 2).sum())
