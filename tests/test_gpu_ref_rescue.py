"""mecat2ref's rescue stage on the device (mecat_amd/csrc/ref_rescue.hip): ref_rescue_prep and ref_rescue_finish through their debug entry
points against what the UNMODIFIED rescue_clipped_align / output_results recorded (tests/golden/ref_rescue.npz) and, beyond the fixture,
against the restatement tests/ref_rescue_ref.py, which tests/test_ref_rescue_cpu.py pins to the same fixture."""
import numpy as np
import pytest

import ref_rescue_cases as SC
import ref_rescue_ref as S

pytestmark = pytest.mark.gpu

MAXC = 10
TRIES = 6


@pytest.fixture(scope="module")
def dev():
    import mecat_amd.hip as M
    ctx = M.Context(0)
    yield dict(M=M, ctx=ctx, fx=SC.fixture())
    ctx.close()


def result_rows(M, entries, qs, slots=None, maxc=MAXC):
    """entries [(qoff, qend, qdir, soff, send)] as one read's first list: entry t in slot slots[t] (t; ascending, ids follow the list), every other
    slot not ok"""
    row = np.zeros(maxc, dtype=M.REF_RESULT_DTYPE)
    # (what a slot that is not ok holds must not matter)
    row["qb"], row["qe"], row["qs"], row["sb"], row["se"] = 0, 99999, 7, 1, 99999
    for t, e in enumerate(entries):
        r = row[slots[t] if slots is not None else t]
        r["ok"], r["qb"], r["qe"], r["chain"], r["sb"], r["se"], r["qs"], r["cols"] = 1, e[0], e[1], e[2], e[3], e[4], qs, 1000
    return row


def rescue_rows(M, tries):
    """tries [(owner, side, result dict or None)] -> (count, meta int32[6], rows [6])"""
    meta = np.zeros(TRIES, dtype=np.int32)
    rows = np.zeros(TRIES, dtype=M.REF_RESULT_DTYPE)
    for j, (owner, side, r) in enumerate(tries):
        meta[j] = owner | side << 8
        if r is not None:
            rows[j]["ok"], rows[j]["qb"], rows[j]["qe"], rows[j]["chain"], rows[j]["sb"], rows[j]["se"] = 1, r["qb"], r["qe"], r["chain"], r["sb"], r["se"]
    return len(tries), meta, rows


def expected(entries, slots, qs, tries, num_output, maxc=MAXC):
    """the restatement's answer for one read -> (state tuple, printed slots)"""
    slots = list(range(len(entries))) if slots is None else slots
    v, go_on = S.prep([S.entry(*e, t) for t, e in enumerate(entries)], qs)
    state = (len(v), int(go_on), len(entries), qs if entries else 0, [slots[a["id"]] for a in v], [a["id"] for a in v])
    after, _ = S.finish(v, go_on, len(entries), qs, tries)
    slot_of = {t: s for t, s in enumerate(slots)}
    nid = len(entries)
    for j, (_, _, r) in enumerate(tries):
        if r is not None:
            slot_of[nid] = maxc + j
            nid += 1
    return state, [slot_of[i] for i in S.output_ids(after, num_output)]


def state_tuple(st):
    n = int(st["naln"])
    assert (st["slot"][n:] == -1).all() and (st["id"][n:] == -1).all()
    return (n, int(st["go_on"]), int(st["nres"]), int(st["qs"]), st["slot"][:n].tolist(), st["id"][:n].tolist())


def run_reads(dev, reads, num_output=10, maxc=MAXC):
    """reads: [(entries, slots, qs, tries)] through prep and finish -> nothing; asserts both kernels against the restatement"""
    M, ctx = dev["M"], dev["ctx"]
    p = M.ref_rescue_params(0, num_output=num_output, maxc=maxc)
    res = np.stack([result_rows(M, e, qs, sl, maxc) for e, sl, qs, _ in reads])
    st = M.debug_ref_rescue_prep(ctx, p, res)
    want = [expected(e, sl, qs, tr, num_output, maxc) for e, sl, qs, tr in reads]
    for i, w in enumerate(want):
        assert state_tuple(st[i]) == w[0], (i, state_tuple(st[i]), w[0])
    rr = [rescue_rows(M, tr if w[0][1] else []) for (_, _, _, tr), w in zip(reads, want)]
    slots, counts = M.debug_ref_rescue_finish(ctx, p, res, st, [r[0] for r in rr], np.stack([r[1] for r in rr]), np.stack([r[2] for r in rr]))
    for i, w in enumerate(want):
        got = slots[i, :counts[i]].tolist()
        assert got == w[1] and (slots[i, counts[i]:] == -1).all(), (i, got, w[1])
    return st, slots, counts


def recorded_tries(c):
    """the searches' outcome of a fixture case in call order, from the recorded results: every recorded candidate gave an ok result, so
    the owners and sides are the restatement's searches' and the results the tool's"""
    qs = len(c["read"])
    v, go_on = S.prep([S.entry(*e, t) for t, e in enumerate(c["entries"])], qs)
    if not go_on:
        return []
    found = S.searches(v, (c["fwd"], c["rev"]), c["block_size"], qs, len(SC.fixture()["ref_codes"]), c["bc"], 0.25)
    assert len(found) == len(c["new"]), c["name"]
    F = {n: i for i, n in enumerate(SC.NEW_FIELDS)}
    return [(o, s, dict(qb=int(r[F["qb"]]), qe=int(r[F["qe"]]), chain=int(r[F["chain"]]), sb=int(r[F["sb"]]), se=int(r[F["se"]]))) for (o, s, _), r in zip(found, c["new"])]


def test_fixture_cases_equal_the_tool(dev):
    """every recorded call: the states of :328-341 and the printed records, at the case's own num_output"""
    cases = dev["fx"]["cases"]
    for no in sorted({c["num_output"] for c in cases}):
        group = [c for c in cases if c["num_output"] == no]
        reads = [(c["entries"], None, len(c["read"]), recorded_tries(c)) for c in group]
        st, slots, counts = run_reads(dev, reads, num_output=no)
        for i, c in enumerate(group):
            # against the recording itself: ids of the first list are their slots here, the k-th result the call added is rescue slot k
            n0 = len(c["entries"])
            want = [i_ if i_ < n0 else MAXC + (i_ - n0) for i_ in c["printed"]]
            assert slots[i, :counts[i]].tolist() == want, c["name"]
            if c["fwd"] or c["rev"]:          # (the one case with seeds in reach where the tool returns before it looks for them)
                assert int(st[i]["go_on"]) == int(c["name"] != "full_edge_19800"), c["name"]


def test_slots_ids_and_lists_shorter_than_ten(dev):
    """the ok results lie anywhere in the list: ids count the ok ones, records are named by slot; maxc below 10"""
    ties = next(c for c in dev["fx"]["cases"] if c["name"] == "ties10")["entries"]
    att = next(c for c in dev["fx"]["cases"] if c["name"] == "attached_then_unattached")
    reads = [(ties[:5], [1, 3, 4, 7, 9], 10000, []), (ties[2:6], [0, 2, 5, 9], 10000, []), (att["entries"], [2, 8], len(att["read"]), recorded_tries(att)), ([], None, 0, [])]
    run_reads(dev, reads)
    run_reads(dev, [(ties[:3], [0, 2, 3], 10000, []), (ties[4:5], [1], 10000, [])], maxc=4, num_output=2)
    run_reads(dev, [(ties[:1], None, 10000, [])], maxc=1, num_output=1)


def test_prep_edges_against_the_restatement(dev):
    """equal lengths, the four containment comparisons at equality and one off, 0.9 of the read at the edge, the other strand"""
    a = (1000, 5000, 0, 20000, 24000)
    reads = []
    for field, lo in ((0, 900), (1, 5100), (3, 19900), (4, 24100)):
        for d in (0, 1):
            b = [1500, 4500, 0, 20500, 23500]
            b[field] = lo - d if field in (0, 3) else lo + d
            reads.append(([tuple(b), a], [4, 6], 9000, []))
    reads.append(([(1100, 4900, 1, 20100, 23900), a], None, 9000, []))
    for qs in (1000, 1001, 1111, 1112):          # 0.9 * qs = 900, 900.9, 999.9, 1000.8 against a length of 900 / 1000
        reads.append(([(50, 950, 0, 100, 1000)], None, qs, []))
        reads.append(([(0, 1000, 0, 100, 1100)], None, qs, []))
    rng = np.random.default_rng(7)
    for _ in range(40):          # random lists with many equal lengths and near-contained pairs
        n = int(rng.integers(1, 11))
        ent = []
        for _t in range(n):
            q0, s0 = int(rng.integers(0, 4)) * 100, int(rng.integers(0, 4)) * 100
            ln = int(rng.integers(10, 14)) * 100
            ent.append((q0, q0 + ln, int(rng.integers(0, 2)), s0, s0 + ln + int(rng.integers(-1, 2)) * 100))
        reads.append((ent, sorted(rng.permutation(MAXC)[:n].tolist()), int(rng.choice([1400, 1445, 3000])), []))
    run_reads(dev, reads)


def attach_cases():
    """hand-made states for the finish kernel: the +-200 and 10 000 bounds of both attach tests at equality and one off, the other
    strand, a rescue result that is not ok, an ok one that is not attached (its id is used), step 6's cut"""
    qs = 30000
    a = (12000, 15000, 0, 40000, 43000)
    reads = []

    def b_left(dq, ds, chain=0):          # b.qend - a.qoff = dq, a.soff - b.send = ds
        return dict(qb=a[0] + dq - 1500, qe=a[0] + dq, chain=chain, sb=a[3] - ds - 1500, se=a[3] - ds)

    def b_right(dq, ds, chain=0):         # a.qend - b.qoff = dq, b.soff - a.send = ds
        return dict(qb=a[1] - dq, qe=a[1] - dq + 1500, chain=chain, sb=a[4] + ds, se=a[4] + ds + 1500)
    for mk, side in ((b_left, 0), (b_right, 1)):
        for dq in (200, 201, -200, -201, 0):
            for ds in (-200, -199, 9999, 10000, 5):
                reads.append(([a], None, qs, [(0, side, mk(dq, ds))]))
        reads.append(([a], None, qs, [(0, side, mk(0, 5, chain=1))]))
    # the second clause: reference ends within 200, the read-side gap inside (-200, 10000)
    for ds in (200, 201, -200, -201):
        for dq in (-200, -199, 9999, 10000):
            reads.append(([a], None, qs, [(0, 0, dict(qb=a[0] - dq - 1200, qe=a[0] - dq, chain=0, sb=a[3] + ds - 1200, se=a[3] + ds))]))
            reads.append(([a], None, qs, [(0, 1, dict(qb=a[1] + dq, qe=a[1] + dq + 1200, chain=0, sb=a[4] - ds, se=a[4] - ds + 1200))]))
    # three entries, six tries: not ok, ok and unattached, attached, in every place
    ents = [a, (2500, 5000, 0, 10000, 12500), (20000, 22000, 0, 60000, 62000)]
    far = dict(qb=100, qe=1300, chain=0, sb=90000, se=91200)
    for mask in range(0, 729, 7):
        tries = []
        for j in range(6):
            o, side = j // 2, j % 2
            e = ents[o]
            kind = (mask // 3 ** j) % 3
            near = (dict(qb=e[0] - 1100, qe=e[0], chain=0, sb=e[3] - 1100, se=e[3]) if side == 0 else dict(qb=e[1], qe=e[1] + 1100, chain=0, sb=e[4], se=e[4] + 1100))
            tries.append((o, side, None if kind == 0 else far if kind == 1 else near))
        reads.append((ents, [1, 4, 7], qs, tries))
        reads.append((ents, [1, 4, 7], qs, tries[1:4]))
    # step 6: an attached result that covers 0.9 of the read (at the edge and one below), alone and beside a second attached one
    for qs2, ln in ((10000, 9000), (10000, 8999), (10001, 9001), (10001, 9000)):
        e = (9200, qs2, 0, 42500, 42500 + qs2 - 9200)
        big = dict(qb=9200 - ln, qe=9200, chain=0, sb=42000 - ln, se=42000)
        reads.append(([e], None, qs2, [(0, 0, big)]))
        e2 = (3000, 3700, 0, 70000, 70700)          # (shorter than e: it sorts behind it)
        reads.append(([e, e2], None, qs2, [(0, 0, big), (1, 0, dict(qb=1900, qe=3000, chain=0, sb=68900, se=70000)), (1, 1, dict(qb=3700, qe=4900, chain=0, sb=70700, se=71900))]))
    return reads


def test_finish_edges_against_the_restatement(dev):
    reads = attach_cases()
    st, slots, counts = run_reads(dev, reads)
    assert (counts == 1).any() and (counts >= 3).any()
    for no in (1, 2):
        run_reads(dev, reads[-40:], num_output=no)


def test_refusals_leave_the_context_working(dev):
    M, ctx = dev["M"], dev["ctx"]
    for kw in (dict(tech=1), dict(maxc=11), dict(maxc=0), dict(num_output=0)):
        p = M.ref_rescue_params(**dict(dict(tech=0), **kw))
        with pytest.raises(M.MhipError):
            M.debug_ref_rescue_prep(ctx, p, np.zeros((1, p.maxc), dtype=M.REF_RESULT_DTYPE))
    # a state that no prep gives
    p = M.ref_rescue_params(0)
    st = np.zeros(1, dtype=M.REF_RESCUE_STATE_DTYPE)
    st["naln"], st["nres"] = 3, 2
    with pytest.raises(M.MhipError):
        M.debug_ref_rescue_finish(ctx, p, np.zeros((1, MAXC), dtype=M.REF_RESULT_DTYPE), st, [0], np.zeros((1, TRIES), dtype=np.int32), np.zeros((1, TRIES), dtype=M.REF_RESULT_DTYPE))
    run_reads(dev, [([(0, 3000, 0, 100, 3100)], None, 5000, [])])
