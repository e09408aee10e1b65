"""dw_extend2's two fast d-row loops after profiles/dw_row_latency.md, read in the compiler's gfx950 listing (no GPU needed, only hipcc; the
file is compiled once).  The loops are found and priced the way test_dw_row_cycles_cpu.fast_row_loops does it; the parts of that write-up
that are in the source are held here, each by its own check:

* 1(a), the snake step's minimum in 16 bits: every snake loop takes nn with one v_min_u16 and holds no v_min_i32;
* 1(b), pass 2's y as x - mk_l and a literal add: the two-pass loop holds no `v_sub_u32 v, 0, v` (the negated diagonal, once per row) and
  no v_add3_u32 with a scalar operand (y from it); pass 2's start point adds the literal 0xffffff80;
* 1(a) + 1(b): 124 - 2 = 122 listed cycles for the one-pass row, 196 - 4 - 2 = 190 for the two-pass row, on dw_extend2<false>, which
  the caps are derived for (the parent listed 124 / 196, tests/test_dw_ring_linear_cpu.py);
* 2, pass 2's ring reads requested at the top of the row: all four ds_read_i16 of a two-pass row stand in front of the first snake loop's
  header, pass 1's two first.  The two early reads are an asm statement, so the compiler does not know that their results are in flight:
  what makes them arrive in time is the wait in front of pass 1's v_max_i16, which takes the last of pass 1's two reads — LDS returns in
  order, so a wait that covers that read covers the two behind it.  The check: between the early reads and that v_max_i16 no instruction
  names their two result registers (a copy there would copy what the register held before), and a wait on lgkmcnt stands in between."""
import os
import re
import subprocess

import pytest

import test_dw_row_cycles_cpu as R
import test_dw_row_scalar_cpu as S

CAP_ONE_PASS, CAP_TWO_PASS = 122, 190

pytestmark = pytest.mark.skipif(not os.path.exists(R.HIPCC), reason="no hipcc")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = tmp_path_factory.mktemp("dwlat") / "dw_extend2.s"
    r = subprocess.run([R.HIPCC] + R._hipflags() + ["-x", "hip", "--cuda-device-only", "-S", os.path.join("mecat_amd", "csrc", "dw_extend2.hip"),
                                                    "-o", str(out)], cwd=R.ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


@pytest.fixture(scope="module", params=sorted(S.KERNELS))
def rows(request, listing):
    """{1: instructions of the one-pass loop, 2: of the two-pass loop} of one instance of the kernel, and its snake loops' headers"""
    kernel = S.KERNELS[request.param]
    found = R.fast_row_loops(listing, kernel)
    assert sorted(found) == [1, 2], "expected the one-pass and the two-pass loop, found %s" % found
    return {n: S.loop_instructions(listing, found[n][0], kernel) for n in (1, 2)}


def _snake_loops(ins):
    """the instruction ranges [first, last] of the snake loops of a row loop: each ends at the branch back behind a snake_step_end, and starts
    at the v_min3_i32's window (the nearest v_sub_u32 pair in front of it)"""
    out = []
    ends = [i for i, (op, a) in enumerate(ins) if op == "s_cbranch_scc1" and i >= 2 and any(o == "s_cmp_lg_u64" for o, _ in ins[i - 3:i])]
    for e in ends:
        lim = [i for i in range(e) if ins[i][0] == "v_min3_i32"]
        if lim and all(x[1] < lim[-1] for x in out):
            out.append((lim[-1], e))
    return out


def test_row_cycles(listing):
    found = R.fast_row_loops(listing, S.KERNELS["pw"])
    print(found)
    assert found[1][2] <= CAP_ONE_PASS, found[1]
    assert found[2][2] <= CAP_TWO_PASS, found[2]


def test_snake_minimum_in_16_bits(rows):
    for n in (1, 2):
        ops = [op for op, _ in rows[n]]
        assert ops.count("v_min_u16") == n, (n, ops.count("v_min_u16"))
        assert not [op for op in ops if op.startswith("v_min_i32")], n
        snakes = _snake_loops(rows[n])
        assert len(snakes) == n, snakes
        for a, b in snakes:
            assert [op for op, _ in rows[n][a:b]].count("v_min_u16") == 1, rows[n][a:b]


def test_pass_two_start_point_without_the_negated_diagonal(rows):
    ins = rows[2]
    neg = [(op, a) for op, a in ins if op.startswith("v_sub_u32") and re.match(r"v\d+, 0, v\d+$", a)]
    assert not neg, neg
    add3 = [(op, a) for op, a in ins if op == "v_add3_u32" and R.isa_mix.classify(op, a) == "valu4" and re.search(r"(?<![a-z0-9_])s\d+", a)]
    assert not add3, add3
    snakes = _snake_loops(ins)
    between = ins[snakes[0][1]:snakes[1][0]]
    lit = [(op, a) for op, a in between if op.startswith("v_add_u32") and "0xffffff80" in a]
    assert len(lit) == 1, between


def test_pass_two_ring_reads_at_the_top_of_the_row(rows):
    ins = rows[2]
    snakes = _snake_loops(ins)
    reads = [i for i, (op, _) in enumerate(ins) if op == "ds_read_i16"]
    assert len(reads) == 4, [ins[i] for i in reads]
    assert reads[-1] < snakes[0][0], "a ring read behind the first snake loop's header: %s" % [ins[i] for i in reads]
    offs = [re.search(r"offset:(\d+)", ins[i][1]) for i in reads]
    assert [int(m.group(1)) if m else 0 for m in offs] == [0, 2, 64, 66], [ins[i] for i in reads]
    # pass 1's v_max_i16 takes its second read; nothing in front of it names the early reads' results, and a wait stands in between
    early = [ins[i][1].split(",")[0].strip() for i in reads[2:]]
    second = ins[reads[1]][1].split(",")[0].strip()
    use = [i for i in range(reads[-1] + 1, snakes[0][0]) if ins[i][0] == "v_max_i16" and second in [x.strip() for x in ins[i][1].split(",")][1:]]
    assert use, "pass 1's v_max_i16 is not between the reads and its snake loop"
    mid = ins[reads[-1] + 1:use[0]]
    named = [(op, a) for op, a in mid if any(re.search(r"(?<![0-9a-z\[:])%s(?![0-9])" % r, a) for r in early)]
    assert not named, "the early reads' results %s are named before they have arrived: %s" % (early, named)
    assert any(op == "s_waitcnt" and "lgkmcnt" in a for op, a in mid), mid
