"""Scalar instructions of dw_extend2's two fast d-row loops, counted in the compiler's gfx950 listing (no GPU needed, only hipcc).

The kernel's scalar side runs at 78 % of the device's measured scalar issue rate (profiles/dw_scalar_side.md), so the scalar instructions
of a row are counted like its vector cycles.  The loops are found the way test_dw_row_cycles_cpu.fast_row_loops finds them: the depth-3
loops that hold the half-wave row maximum (v_permlane16_swap), the one-pass loop with one snake loop nested in it, the two-pass loop with
two.  Counted are the `salu`-class instructions (isa_mix.classify) of every block of the loop as listed, the rare part of snake_step_end
included; branches, waits and nops are classes of their own.

The parent of the commit that added this test listed 31 scalar instructions in the one-pass loop and 58 in the two-pass loop.  Derived
from that listing (profiles/dw_scalar_side.md):

* S1, two-pass row: both passes' lane masks from one s_bfm_b64 per half and three moves (one word is formed in place), where twelve
  instructions stood: -7;
* S2, two-pass band update: the two 64-bit words by three moves instead of five moves and two s_or_b64 (-4), slots as
  65 - (ctz + clz) (-2): -6.

58 - 7 - 6 = 45 for the two-pass loop, which is what the compiler lists; the one-pass loop keeps its 31.  The caps leave two for
scheduling differences, as the caps of the vector cycles do.  Not in the source, so not in the caps or the forms: S3 (the one-pass loop
bound at 31 slots, without s_bitcmp0_b32, the `full` test on a peeled row: 28 listed, measured 1.5 ms slower), S4 (the snake loop's
re-test of `more`: the compiler does not take the form) and S5 (the two-pass loop test from the pass-2 masks: 44 listed and one branch
more, measured level).  The forms of the kept steps are asserted next to the counts, on both instances of the kernel."""
import os
import re
import subprocess

import pytest

import test_dw_row_cycles_cpu as R

CAP_ONE_PASS, CAP_TWO_PASS = 33, 47
KERNELS = {"pw": "_Z10dw_extend2ILb0E", "cns": "_Z10dw_extend2ILb1E"}

pytestmark = pytest.mark.skipif(not os.path.exists(R.HIPCC), reason="no hipcc")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = tmp_path_factory.mktemp("dwsalu") / "dw_extend2.s"
    r = subprocess.run([R.HIPCC] + R._hipflags() + ["-x", "hip", "--cuda-device-only", "-S", os.path.join("mecat_amd", "csrc", "dw_extend2.hip"),
                                                    "-o", str(out)], cwd=R.ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def loop_instructions(text, header, kernel):
    """[(mnemonic, operands)] of every block of `kernel` that belongs to the loop headed by `header` or to a loop nested in it, in
    listing order (the listing's own loop annotations, read as fast_row_loops reads them)"""
    m = re.search(r"^%s\w*:.*?^\s*s_endpgm" % kernel, text, re.M | re.S)
    assert m, "kernel not in the listing"
    blocks = re.split(r"^(?=\.LBB\d+_\d+:|; %bb\.\d+:)", m.group(0), flags=re.M)
    parent = {}
    for b in blocks:
        lab = re.match(r"\.L(BB\d+_\d+):", b)
        head = "\n".join(b.splitlines()[:16])
        if lab and re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=\d+", head):
            ps = [(int(d), h) for h, d in re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", head)]
            parent[lab.group(1)] = max(ps)[1] if ps else None
    out = []
    for b in blocks:
        first = b.splitlines()[0] if b else ""
        lab = re.match(r"\.L(BB\d+_\d+):", b)
        mi = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=\d+", first)
        h = lab.group(1) if lab and lab.group(1) in parent else mi.group(1) if mi else None
        while h and h != header:
            h = parent.get(h)
        if h != header:
            continue
        for ln in b.splitlines()[1:]:
            s = ln.split(";")[0].strip()
            mo = re.match(r"([a-z_0-9]+)\s*(.*)", s)
            if s and not s.endswith(":") and not s.startswith(".") and mo:
                out.append((mo.group(1), mo.group(2)))
    return out


@pytest.fixture(scope="module", params=sorted(KERNELS))
def rows(request, listing):
    """{1: instructions of the one-pass loop, 2: of the two-pass loop} of one instance of the kernel"""
    kernel = KERNELS[request.param]
    found = R.fast_row_loops(listing, kernel)
    assert sorted(found) == [1, 2], "expected the one-pass and the two-pass loop, found %s" % found
    out = {n: loop_instructions(listing, found[n][0], kernel) for n in (1, 2)}
    for n in (1, 2):
        assert sum(1 for op, _ in out[n] if op.startswith("v_permlane16_swap")) == 1, "loop %s is not one row" % found[n][0]
    print(request.param, {n: salu(out[n]) for n in out})
    return out


def salu(ins):
    return sum(1 for op, args in ins if R.isa_mix.classify(op, args) == "salu")


def test_one_pass_row_scalar_count(rows):
    assert salu(rows[1]) <= CAP_ONE_PASS, [i for i in rows[1] if i[0].startswith("s_")]


def test_two_pass_row_scalar_count(rows):
    assert salu(rows[2]) <= CAP_TWO_PASS, [i for i in rows[2] if i[0].startswith("s_")]


def test_two_pass_row_masks_and_words(rows):
    ops = [op for op, _ in rows[2]]
    assert ops.count("s_bfm_b64") <= 2, "one s_bfm_b64 per half serves both passes"
    # the band update: behind the two ballots of the threshold compare, the words of the two halves reach the find-first without an OR
    cmp = [i for i, op in enumerate(ops) if op.startswith("v_cmp_ge")]
    ff1 = [i for i, op in enumerate(ops) if op == "s_ff1_i32_b64"]
    assert len(cmp) >= 2 and len(ff1) == 2, (cmp, ff1)
    assert cmp[-2] < ff1[0], (cmp, ff1)
    between = ops[cmp[-2]:ff1[0]]
    assert "s_or_b64" not in between, between
