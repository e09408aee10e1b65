"""Plain restatement of what mecat2ref does with a read's results between its extension loop and the result file (PacBio mode):
rescue_clipped_align (mecat2ref/mecat2ref_aux.cpp:308-452) with its helpers (:185-306, mecat2ref_aux.h:22-42) and output_results
(:454-473).  It stands on tests/ref_cand_ref.py (find_location) and tests/ref_ext_ref.py (the extension); tests/test_ref_rescue_cpu.py
pins it to what the unmodified functions recorded (tests/golden/ref_rescue.npz).

An entry is a dict(qoff, qend, qdir (0 'F' / 1 'R'), soff, send, id, prev_id, next_id, parent_id); `id` is the index of the result among
the read's results, as extend_candidate counts them.  A database is {segment: (score2, loczhi[<= 20], seedno[<= 20])}; a segment that
is not in it has score2 0."""
import ref_cand_ref as R

CLIPPED = 2000
SM = 20
TRIES = 6


def entry(qoff, qend, qdir, soff, send, id_):
    return dict(qoff=int(qoff), qend=int(qend), qdir=int(qdir), soff=int(soff), send=int(send), id=int(id_), prev_id=-1, next_id=-1, parent_id=-1)


def is_full(a, qsize):
    return a["qend"] - a["qoff"] >= qsize * 0.9


def contained(a, b, extra=100):
    return (a["qdir"] == b["qdir"] and b["qoff"] + extra >= a["qoff"] and b["qend"] <= a["qend"] + extra and b["soff"] + extra >= a["soff"]
            and b["send"] <= a["send"] + extra)


def is_left_clipped(a, b):
    if a["qdir"] != b["qdir"]:
        return False
    if abs(b["qend"] - a["qoff"]) <= 200 and -200 < a["soff"] - b["send"] < 10000:
        return True
    return abs(b["send"] - a["soff"]) <= 200 and -200 < a["qoff"] - b["qend"] < 10000


def is_right_clipped(a, b):
    if a["qdir"] != b["qdir"]:
        return False
    if abs(a["qend"] - b["qoff"]) <= 200 and -200 < b["soff"] - a["send"] < 10000:
        return True
    return abs(a["send"] - b["soff"]) <= 200 and -200 < b["qoff"] - a["qend"] < 10000


def sort_entries(v):
    """std::sort with AlignInfo's operator< on at most 16 elements: libstdc++'s insertion sort, so equal lengths keep their order"""
    assert len(v) <= 16
    return sorted(v, key=lambda a: -(a["qend"] - a["qoff"]))          # (Python's sort is stable)


def prep(entries, qsize):
    """:328-341 -> (the surviving entries in order, go_on)"""
    v = sort_entries(entries)
    valid = [True] * len(v)
    for i in range(len(v) - 1):
        if not valid[i]:
            continue
        for j in range(i + 1, len(v)):
            if valid[j] and contained(v[i], v[j]):
                valid[j] = False
    v = [a for a, ok in zip(v, valid) if ok]
    return v, bool(v) and not is_full(v[0], qsize)


def _fill(db, bid, chain, read_size, bc, block_size, cutoff):
    """fill_clipped_candidate (:185-212) -> None or dict(score, chain, loc1, loc2)"""
    score2, loczhi, seedno = db[bid]
    n = min(score2, SM)
    f = R._find_location([int(x) for x in loczhi[:n]], [int(x) for x in seedno[:n]], bc, read_size, cutoff)
    if f is None:
        return None
    loc0, seed0, rep_loc, sc = f
    return dict(score=int(sc[rep_loc]), chain=chain, loc1=bid * block_size + loc0, loc2=(seed0 - 1) * bc)


def _best(db, segs):
    """the scanned segment with the largest score2, the first met winning (`>`), None when all are 0"""
    best, bid = 0, None
    for s in segs:
        sc = db[s][0] if s in db else 0
        if sc > best:
            best, bid = sc, s
    return bid


def find_left(a, db, block_size, read_size, bc, cutoff):
    """find_left_clipped_candidate (:214-242)"""
    if a["qoff"] <= CLIPPED or a["soff"] <= CLIPPED:
        return None
    n2 = a["soff"] // block_size
    n = min(a["qoff"] // block_size, n2)
    segs = []
    n2 -= 1
    while n >= 0 and n2 >= 0:
        segs.append(n2)
        n -= 1
        n2 -= 1
    bid = _best(db, segs)
    if bid is None or not db[bid][0] > 4:
        return None
    return _fill(db, bid, a["qdir"], read_size, bc, block_size, cutoff)


def find_right(a, db, block_size, read_size, ref_size, bc, cutoff):
    """find_right_clipped_candidate (:244-274)"""
    if read_size - a["qend"] <= CLIPPED or ref_size - a["send"] <= CLIPPED:
        return None
    n = min((read_size - a["qend"]) // block_size, (ref_size - a["send"]) // block_size)
    k = a["send"] // block_size + 1
    bid = _best(db, range(k, k + n + 1))
    if bid is None or not db[bid][0] > 4:
        return None
    return _fill(db, bid, a["qdir"], read_size, bc, block_size, cutoff)


def searches(v, dbs, block_size, read_size, ref_size, bc, cutoff):
    """the tool's calls in order for the first three entries -> [(owner, side, candidate)] (at most 6); side 0 left, 1 right.  The
    searches read nothing the attach step writes (an entry's prev_id / next_id are set by its own side only), so they can all run
    before the first extension"""
    out = []
    for i, a in enumerate(v[:3]):
        db = dbs[a["qdir"]]
        c = find_left(a, db, block_size, read_size, bc, cutoff)
        if c is not None:
            out.append((i, 0, c))
        c = find_right(a, db, block_size, read_size, ref_size, bc, cutoff)
        if c is not None:
            out.append((i, 1, c))
    return out


def finish(v, go_on, nres, qsize, tries):
    """:359-451 behind the searches.  v: prep's entries; nres: the results the read has so far; tries: [(owner, side, result)] in call
    order, result = None (the extension gave nothing) or dict(qb, qe, chain, sb, se) -> (entries, results after the call)"""
    v = [dict(a) for a in v]
    if not go_on:
        return v, nres
    k = 0
    for owner, side, r in tries:
        if r is None:
            continue
        ai = entry(r["qb"], r["qe"], r["chain"], r["sb"], r["se"], nres)
        nres += 1
        a = v[owner]
        if (is_right_clipped if side else is_left_clipped)(a, ai):
            ai["parent_id"] = a["id"]
            a["next_id" if side else "prev_id"] = ai["id"]
            v.append(ai)
            k += 1
    if not k:          # (an ok result that was not attached left no entry: the tool overwrites it; its id stays used)
        return v, nres
    v = sort_entries(v)
    full = [a for a in v if is_full(a, qsize)]
    if full:
        for a in full:
            a["parent_id"] = a["prev_id"] = a["next_id"] = -1
        v = v[:len(full)]
    return v, nres


def output_ids(v, num_output):
    """output_results -> the ids in the order their records are printed"""
    out, n = [], 0
    for a in v:
        if n >= num_output:
            break
        if a["parent_id"] != -1:
            continue
        out.append(a["id"])
        if a["prev_id"] != -1:
            out.append(a["prev_id"])
        if a["next_id"] != -1:
            out.append(a["next_id"])
        n += 1
    return out


# ---- the segment records the searches read, and the whole stage for one read
def seed_records(idx, seq, rnd, cutoff):
    """the seeding loop of reference_mapping (mecat2ref_impl_large.cpp:417-453, insert_loc :92-130) for one strand's letters -> the
    database {segment: (score2, loczhi, seedno)}.  It is the loop at the head of tests/ref_cand_ref.py's strand_stream, restated here
    because that function hands back candidates only; `score2` is the score this loop leaves (:448), before the candidate phase zeroes
    some"""
    L = len(seq)
    if L < R.K:
        return {}
    bc = 5 if rnd else min(20, 5 + L // 1000)
    Z = 2000 if rnd else 1000
    num = (L - R.K) // bc + 1
    ids = R.kmer_ids(seq)[: (num - 1) * bc + 1: bc]
    st, cn = idx.buckets(ids)
    db = {}
    for k in (i for i, c in enumerate(cn.tolist()) if c):
        for p in idx.pos[st[k]: st[k] + cn[k]].tolist():
            seg, off = divmod(p, Z)
            r = db.get(seg)
            if r is None:
                r = db[seg] = R._Seg()
            if r.score == 0 or r.seednum < k + 1:
                r.score += 1
                if r.score <= SM:
                    r.loc.append(off)
                    r.seed.append(k + 1)
                else:
                    R._insert_loc(r, off, k + 1, bc, cutoff)
            r.seednum = k + 1
    return {seg: (r.score, list(r.loc), list(r.seed)) for seg, r in db.items()}


def rescue_read(first, qsize, num_output, database, extend, block_size, ref_size, bc, cutoff):
    """the whole stage for one read.  first: the read's ok results in list order, dicts(qb, qe, chain, sb, se); database(strand) -> the
    strand's records (asked for only when an entry of the first three is on it); extend(candidate) -> None or a result dict
    -> dict(go_on, tries [(owner, side, candidate, result)], printed ids, nresults)"""
    v, go_on = prep([entry(r["qb"], r["qe"], r["chain"], r["sb"], r["se"], t) for t, r in enumerate(first)], qsize)
    tries = []
    if go_on:
        dbs = {s: database(s) for s in {a["qdir"] for a in v[:3]}}
        for owner, side, cand in searches(v, dbs, block_size, qsize, ref_size, bc, cutoff):
            tries.append((owner, side, cand, extend(cand)))
    after, nres = finish(v, go_on, len(first), qsize, [(o, s, r) for o, s, _, r in tries])
    return dict(go_on=go_on, tries=tries, printed=output_ids(after, num_output), nresults=nres, after=after)
