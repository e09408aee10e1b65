"""A plain numpy statement of mecat2cns' consensus table rules, for the tests of the device table (mecat_amd/csrc/cns_table.hip).

Written from the rules, not from the reference's loop; test_cns_table_ref_cpu.py pins it against hand-computed tables and against what the
compiled, unmodified reference gives (tests/golden/cns_table.npz: meap_add_one_aln on adversarial pairs, every ident byte).

One alignment is two equally long strings over "ACGT-" (q: the query read, s: the template) and `soff`, the template position of the
first template base.  The template position of column i is

    p(i) = soff + number of columns before i whose s character is not '-'

and a column adds to the template's table {mat_cnt, ins_cnt, del_cnt}:

    q '-' and s '-'          nothing
    q == s, both bases       mat_cnt[p(i)] += 1
    q '-', s a base          ins_cnt[p(i)] += 1
    s '-'                    belongs to a maximal run of consecutive columns whose s is '-'; the whole run adds one
                             del_cnt[p(first column of the run) - 1] += 1 if at least one of its columns has a q base, and nothing
                             when p - 1 would be -1

A column with two different bases is not part of the format (ValueError).  Then, per position, base = the template's letter where
mat_cnt > 0, else 'N', and with cov = mat_cnt + ins_cnt, in double arithmetic:

    ident = FMAT(1) if mat_cnt >= cov * 0.8 | FINS(4) if ins_cnt >= cov * 0.8, UNDS(8) if neither, | FDEL(2) if del_cnt >= cov * 0.4
"""
import numpy as np

GAP = ord("-")
FMAT, FDEL, FINS, UNDS = 1, 2, 4, 8
TABLE_DTYPE = np.dtype([("base", np.uint8), ("mat_cnt", np.uint8), ("ins_cnt", np.uint8), ("del_cnt", np.uint8)])


def _u8(x):
    return np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else x.astype(np.uint8, copy=False)


def tally_one(counts, q, s, soff):
    """adds one alignment to counts (int64 [tmpl_len, 3]: mat, ins, del)"""
    q, s = _u8(q), _u8(s)
    assert len(q) == len(s)
    if len(q) == 0:
        return
    sbase, qbase = s != GAP, q != GAP
    if np.any(sbase & qbase & (q != s)):
        raise ValueError("mismatch column")
    p = soff + np.cumsum(sbase) - sbase          # bases of s in front of every column
    np.add.at(counts[:, 0], p[sbase & qbase], 1)
    np.add.at(counts[:, 1], p[sbase & ~qbase], 1)
    edge = np.diff(np.concatenate([[0], (~sbase).astype(np.int8), [0]]))
    for a, b in zip(np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]):      # maximal s-gap runs: columns [a, b)
        if qbase[a:b].any() and p[a] - 1 >= 0:
            counts[p[a] - 1, 2] += 1


def ident_of(mat, ins, dele):
    out = np.zeros(len(mat), dtype=np.uint8)
    for i, (m, n, d) in enumerate(zip(mat.tolist(), ins.tolist(), dele.tolist())):
        cov = m + n
        v = 0
        if float(m) >= cov * 0.8:
            v |= FMAT
        if float(n) >= cov * 0.8:
            v |= FINS
        if not v:
            v |= UNDS
        if float(d) >= cov * 0.4:
            v |= FDEL
        out[i] = v
    return out


def build_table(alns, tmpl_letters):
    """alns: iterable of (q, s, soff); tmpl_letters: bytes.  -> (table [len] TABLE_DTYPE, ident [len] uint8)"""
    let = _u8(tmpl_letters)
    counts = np.zeros((len(let), 3), dtype=np.int64)
    for q, s, soff in alns:
        tally_one(counts, q, s, int(soff))
    assert counts.max(initial=0) <= 255, "a count does not fit its byte"
    table = np.zeros(len(let), dtype=TABLE_DTYPE)
    table["mat_cnt"], table["ins_cnt"], table["del_cnt"] = counts[:, 0], counts[:, 1], counts[:, 2]
    table["base"] = np.where(counts[:, 0] > 0, let, ord("N"))
    return table, ident_of(counts[:, 0], counts[:, 1], counts[:, 2])


MAX_CNS_OVLPS = 100      # the most alignments mecat2cns gives one template: the largest coverage a table position can have


def sweep_triples(max_cov=MAX_CNS_OVLPS):
    """every (mat, ins, del) a position of the table can hold with mat + ins <= max_cov and del <= mat + ins, in the order of
    tests/golden/cns_table.npz `sweep_ident`: cov = mat + ins ascending, then mat ascending, then del ascending  -> int32 [348 551, 3]"""
    rows = []
    for cov in range(max_cov + 1):
        mat = np.repeat(np.arange(cov + 1), cov + 1)
        dele = np.tile(np.arange(cov + 1), cov + 1)
        rows.append(np.stack([mat, cov - mat, dele], axis=1))
    return np.concatenate(rows).astype(np.int32)
