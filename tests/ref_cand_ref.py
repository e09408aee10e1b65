"""mecat2ref's seeding and candidate selection (the front half of reference_mapping, mecat2ref_impl_large.cpp) restated in plain Python
and numpy from its rules: the expected-value function of mhip_ref_seed_reads for inputs beyond tests/golden/ref_cand.npz, itself pinned
to that fixture by tests/test_ref_cand_cpu.py.

  index       every 13-mer of the reference letters (concatenated, upper-cased) without a letter other than A, C, G, T, 1-based start
              positions ascending per 13-mer, 13-mers with more than 128 occurrences dropped
  seeds       read k-mers at stride BC (round 0: min(20, 5 + len / 1000), round 1: 5), (len - 13) / BC + 1 of them; a k-mer with a letter
              other than upper-case A, C, G, T is skipped; the reverse strand is the reverse complement, other letters kept
  segments    Z = 1 000 (round 0) or 2 000 (round 1) positions, 20 stored seeds, the 21st and later go through insert_loc
  gates       index_score > 6 (round 0) / > 4 (round 1), find_location with maxval >= 5, its vote >= 6
  arithmetic  find_location and insert_loc divide in f32 (int / (int * float)) and compare with the f64 cutoff; the sweeps divide in f64
"""
import numpy as np

SM = 20
K = 13
_CODE = np.full(256, 4, dtype=np.int64)
_CODE[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4)
_COMP = np.arange(256, dtype=np.uint8)
_COMP[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)
_IU = {n: np.triu_indices(n, 1) for n in range(2, 2 * SM + 2)}


def kmer_ids(let):
    """letters -> int64[len - 12]: the 13-mer id at every start (A, C, G, T = 0..3, first letter in the top bits), -1 where the 13-mer
    holds another letter"""
    c = _CODE[np.asarray(let, dtype=np.uint8)]
    n = len(c) - K + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    ids = np.zeros(n, dtype=np.int64)
    bad = np.zeros(n, dtype=bool)
    for j in range(K):
        ids = (ids << 2) | (c[j: j + n] & 3)
        bad |= c[j: j + n] == 4
    ids[bad] = -1
    return ids


def upper(let):
    let = np.asarray(let, dtype=np.uint8).copy()
    let[(let >= ord("a")) & (let <= ord("z"))] -= 32          # creat_ref_index: toupper of a letter above 'Z'
    return let


class Index:
    """creat_ref_index: counts below 129 kept, larger buckets empty; positions 1-based, ascending"""

    def __init__(self, ref_letters):
        ids = kmer_ids(upper(ref_letters))
        pos = np.flatnonzero(ids >= 0)
        order = np.argsort(ids[pos], kind="stable")
        self.keys, first, cnt = np.unique(ids[pos][order], return_index=True, return_counts=True)
        keep = cnt <= 128
        self.keys, self.first, self.cnt = self.keys[keep], first[keep], cnt[keep]
        self.pos = pos[order] + 1
        self.seqcount = len(ref_letters)

    def buckets(self, ids):
        """-> per id (start into self.pos, count); count 0 for a missing or negative id"""
        i = np.searchsorted(self.keys, ids)
        i[i == len(self.keys)] = 0
        hit = (self.keys[i] == ids) if len(self.keys) else np.zeros(len(ids), dtype=bool)
        return np.where(hit, self.first[i], 0), np.where(hit, self.cnt[i], 0)


def revcomp(let):
    return _COMP[np.asarray(let, dtype=np.uint8)[::-1]]


def _pair_votes(ll, ss, bc, cutoff, read_len=None):
    """the pairwise DDF vote over entries (ll, ss): pairs i < j with ss[j] > ss[i], ll[j] > ll[i] (and ll[j] - ll[i] < read_len when
    given) and fabs(f32 quotient - 1) < cutoff -> votes per entry"""
    n = len(ll)
    if n < 2:
        return np.zeros(n, dtype=np.int64)
    iu = _IU[n]
    dl = ll[iu[1]] - ll[iu[0]]
    ds = ss[iu[1]] - ss[iu[0]]
    ok = (ds > 0) & (dl > 0)
    if read_len is not None:
        ok &= dl < read_len
    den = ds.astype(np.float32) * np.float32(bc)
    den[~ok] = np.float32(1)
    q = dl.astype(np.float32) / den
    if read_len is not None:
        ok &= np.abs(q - np.float32(1)).astype(np.float64) < cutoff          # find_location: `- 1`, an f32 subtraction
    else:
        ok &= np.abs(q.astype(np.float64) - 1.0) < cutoff                    # insert_loc: `- 1.0`, an f64 subtraction
    return np.bincount(iu[0][ok], minlength=n) + np.bincount(iu[1][ok], minlength=n)


def _ddf32(dl, ds, bc, cutoff):
    q = np.float32(dl) / (np.float32(ds) * np.float32(bc))
    return abs(float(np.float32(q - np.float32(1)))) < cutoff


class _Seg:
    __slots__ = ("score", "loc", "seed", "seednum", "index")

    def __init__(self):
        self.score, self.loc, self.seed, self.seednum, self.index = 0, [], [], 0, -1


def _insert_loc(r, loc, seedn, bc, cutoff):
    sc = _pair_votes(np.array(r.loc + [loc], dtype=np.int64), np.array(r.seed + [seedn], dtype=np.int64), bc, cutoff)
    minval, mini = int(sc.min()), int(sc.argmin())          # (the first minimum)
    if minval == SM:
        r.loc[SM - 1], r.seed[SM - 1] = loc, seedn
    elif minval < SM and mini < SM:
        del r.loc[mini], r.seed[mini]
        r.loc.append(loc)
        r.seed.append(seedn)
        r.score -= 1


def _find_location(tl, ts, bc, read_len, cutoff):
    """-> None or (loc0, seed0, rep_loc, votes)"""
    k = len(tl)
    sc = _pair_votes(np.array(tl, dtype=np.int64), np.array(ts, dtype=np.int64), bc, cutoff, read_len)
    maxval, maxi, rep = 0, 0, 0
    for i in range(k):
        if maxval < sc[i]:
            maxval, maxi, rep = int(sc[i]), i, 0
        elif maxval == sc[i]:
            rep += 1
    if maxval < 5:
        return None
    if rep == maxval:
        return tl[maxi], ts[maxi], maxi, sc
    loc0, seed0, rep_loc = 0, 0, 0
    for j in range(maxi):
        d = tl[maxi] - tl[j]
        if ts[maxi] - ts[j] > 0 and d > 0 and d < read_len and _ddf32(d, ts[maxi] - ts[j], bc, cutoff) and loc0 == 0:
            loc0, seed0, rep_loc = tl[j], ts[j], j
    if loc0 == 0:
        loc0, seed0, rep_loc = tl[maxi], ts[maxi], maxi
    for j in range(maxi + 1, k):
        d = tl[j] - tl[maxi]
        if ts[j] - ts[maxi] > 0 and d > 0 and d <= read_len and _ddf32(d, ts[j] - ts[maxi], bc, cutoff) and loc0 == 0:
            loc0, seed0, rep_loc = tl[j], ts[j], j
    return loc0, seed0, rep_loc, sc


def strand_stream(idx, seq, rnd, cutoff, chain):
    """one strand's candidates in arrival order: [(loc1, loc2, left1, left2, right1, right2, score, num1, num2, chain)]"""
    L = len(seq)
    if L < K:
        return []
    bc = 5 if rnd else min(20, 5 + L // 1000)
    Z = 2000 if rnd else 1000
    gate = 4 if rnd else 6
    num = (L - K) // bc + 1
    ids = kmer_ids(seq)[: (num - 1) * bc + 1: bc]
    st, cn = idx.buckets(ids)
    pos = idx.pos
    db, order, iscore = {}, [], []
    for k in np.flatnonzero(cn).tolist():
        for p in pos[st[k]: st[k] + cn[k]].tolist():
            seg, off = divmod(p, Z)
            r = db.get(seg)
            if r is None:
                r = db[seg] = _Seg()
            if r.score == 0 or r.seednum < k + 1:
                r.score += 1
                if r.score <= SM:
                    r.loc.append(off)
                    r.seed.append(k + 1)
                else:
                    _insert_loc(r, off, k + 1, bc, cutoff)
                left = db.get(seg - 1)
                sk = r.score + (left.score if left is not None else 0)
                if r.index == -1:
                    r.index = len(order)
                    order.append(seg)
                    iscore.append(sk)
                else:
                    iscore[r.index] = sk
            r.seednum = k + 1
    out = []
    zero = _Seg()
    for i, seg in enumerate(order):
        if not iscore[i] > gate:
            continue
        r = db[seg]
        if r.score == 0:
            continue
        left = db.get(seg - 1, zero)
        if left.score > 0:
            start_loc = (seg - 1) * Z
            nl = min(left.score, SM)
            ns = min(r.score, SM)
            tl = left.loc[:nl] + [x + Z for x in r.loc[:ns]]
            ts = left.seed[:nl] + r.seed[:ns]
        else:
            start_loc = seg * Z
            ns = min(r.score, SM)
            tl, ts = r.loc[:ns], r.seed[:ns]
        f = _find_location(tl, ts, bc, L, cutoff)
        if f is None:
            continue
        loc0, seed0, rep_loc, sc = f
        if sc[rep_loc] < 6:
            continue
        score = int(sc[rep_loc])
        loc_seed = ts[rep_loc]
        loc0 += start_loc
        loc1 = (seed0 - 1) * bc
        left1, right1 = loc0 + K - 1, idx.seqcount - loc0
        left2, right2 = loc1 + K - 1, L - loc1
        num1, num2 = min(left1, left2), min(right1, right2)
        seedcount = 0
        with np.errstate(divide="ignore", invalid="ignore"):
            u, kk = seg - 2, num1 // Z
            while u >= 0 and kk >= 0:
                o = db.get(u)
                if o is not None and o.score > 0:
                    scnt = min(o.score, SM)
                    a = (loc0 - u * Z - np.array(o.loc[:scnt], dtype=np.float64)) / ((loc_seed - np.array(o.seed[:scnt], dtype=np.int64)) * bc * 1.0)
                    s = int((np.abs(a - 1.0) < cutoff).sum())
                    seedcount += s
                    if s * 1.0 / scnt > 0.4:
                        o.score = 0
                u -= 1
                kk -= 1
            u, kk = seg + 1, num2 // Z
            while kk > 0:
                o = db.get(u)
                if o is not None and o.score > 0:
                    scnt = min(o.score, SM)
                    a = (u * Z + np.array(o.loc[:scnt], dtype=np.float64) - loc0) / ((np.array(o.seed[:scnt], dtype=np.int64) - loc_seed) * bc * 1.0)
                    s = int((np.abs(a - 1.0) < cutoff).sum())
                    seedcount += s
                    if s * 1.0 / scnt > 0.4:
                        o.score = 0
                u += 1
                kk -= 1
        out.append((loc0, loc1, left1, left2, right1, right2, score + seedcount, num1, num2, chain))
    return out


def read_stream(idx, read, rnd, cutoff):
    """both strands' candidates of one read in arrival order (forward strand first)"""
    read = np.asarray(read, dtype=np.uint8)
    return strand_stream(idx, read, rnd, cutoff, 0) + strand_stream(idx, revcomp(read), rnd, cutoff, 1)


def insert_list(stream, maxc):
    """the reference's binary insertion by score into a list of at most maxc entries -> int64[count, 10]"""
    lst = []
    for c in stream:
        n = len(lst)
        low, high = 0, n - 1
        while low <= high:
            mid = (low + high) // 2
            if mid >= n or lst[mid][6] < c[6]:
                high = mid - 1
            else:
                low = mid + 1
        if high + 1 < maxc:
            lst.insert(high + 1, c)
            del lst[maxc:]
    return np.array(lst, dtype=np.int64).reshape(-1, 10)


def candidates(idx, read, rnd, cutoff, maxc):
    return insert_list(read_stream(idx, read, rnd, cutoff), maxc)


# ---- the reference file (creat_ref_index's reading of it)
def read_reference(text):
    """FASTA bytes -> (letters concatenated and upper-cased, chrindex.txt bytes)"""
    let, lines, count, rsize = [], [], 0, 0
    started = False
    for ln in bytes(text).split(b"\n"):
        if ln[:1] == b">":
            if rsize:
                lines.append(b"%d\n" % rsize)
            rsize = 0
            name = ln[1:]
            for i, ch in enumerate(name):
                if ch in (32, 9):
                    name = name[:i]
                    break
            lines.append(b"%d\t%s\t" % (count, name))
            started = True
        else:
            s = np.frombuffer(ln.replace(b"\r", b""), dtype=np.uint8)
            let.append(s)
            count += len(s)
            rsize += len(s)
    assert started
    lines.append(b"%d\n" % rsize)
    lines.append(b"%d\tFileEnd\n" % count)
    return upper(np.concatenate(let)), b"".join(lines)


def ref_tables(let):
    """upper-cased reference letters -> (pac, nplane, read table int32[n, 2]) as mecat_amd/host/ref_genome.cpp makes them: pac / nplane
    four letters per byte, first in the top bits; the table's reads are the maximal runs of A, C, G, T, and inside every longer stretch
    of other letters zero-length reads no more than 13 apart, the last one on the stretch's last letter (the index build marks the 13
    positions that end at a read's end, [end - 12, end], as starting no k-mer: together these cover every 13-mer that holds such a
    letter, and no other)"""
    c = _CODE[let]
    n = len(let)
    pad = (-n) % 4
    codes = np.concatenate([np.where(c < 4, c, 0), np.zeros(pad, dtype=np.int64)]).reshape(-1, 4)
    nn = np.concatenate([np.where(c < 4, 0, 3), np.zeros(pad, dtype=np.int64)]).reshape(-1, 4)
    pk = lambda a: (a[:, 0] << 6 | a[:, 1] << 4 | a[:, 2] << 2 | a[:, 3]).astype(np.uint8)
    table = []
    i = 0
    while i < n:
        j = i
        while j < n and c[j] < 4:
            j += 1
        if j > i or i == 0:
            table.append((i, j - i))          # (a reference that starts with another letter starts with an empty read on it)
        if j == n:
            break
        e = j
        while e < n and c[e] == 4:
            e += 1
        # the stretch [j, e): position j is the end of the read in front of it
        p = j
        while p + 13 < e - 1:
            p += 13
            table.append((p, 0))
        if e - 1 > p:
            table.append((e - 1, 0))
        i = e
    return pk(codes), pk(nn), np.array(table, dtype=np.int32).reshape(-1, 2)
