"""Issue cycles of dw_extend2<false>'s two fast d-row loops behind the word-interleaved staging and the single select per pass, priced
from the compiler's gfx950 listing as test_dw_row_cycles_cpu does (its `fast_row_loops`: the listed loop, the rare part of the snake step
included).

The loops stood at 142 cycles per one-pass row and 240 per two-pass row.  Two changes are derived from that listing
(profiles/dw_staging.md):

* the staged words of a workgroup's eight halves are interleaved word-major, so a window's byte offset is x2 & ~31 and its address one
  and-or (query) or an and and an add (target): 4 issue cycles where v_ashrrev_i32 + v_lshl_add_u32 took 6, twice per snake step:
  -4 per pass;
* the register that idle lanes select carries a large negative upper half, so x + y is formed from the one selected value and the second
  v_cndmask of a pass goes: -4 per pass.

142 - 8 = 134 for the one-pass row, 240 - 16 = 224 for the two-pass row.  The caps leave two cycles for scheduling differences, as the
existing caps did.  The removed address form is `v_lshl_add_u32`: no snake loop may contain one."""
import os
import re
import subprocess

import pytest

import test_dw_row_cycles_cpu as R

CAP_ONE_PASS, CAP_TWO_PASS = 136, 226

pytestmark = pytest.mark.skipif(not os.path.exists(R.HIPCC), reason="no hipcc")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = tmp_path_factory.mktemp("dwstg") / "dw_extend2.s"
    r = subprocess.run([R.HIPCC] + R._hipflags() + ["-x", "hip", "--cuda-device-only", "-S", os.path.join("mecat_amd", "csrc", "dw_extend2.hip"),
                                                    "-o", str(out)], cwd=R.ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


@pytest.fixture(scope="module")
def loops(listing):
    found = R.fast_row_loops(listing)
    print(found)
    assert sorted(found) == [1, 2], "expected the one-pass and the two-pass loop, found %s" % found
    return found


def snake_loop_bodies(text, row_headers, kernel=R.KERNEL):
    """{header label: [instruction lines]} of the loops of `kernel` whose parent loop is one of row_headers (the listing's own loop
    annotations: a snake loop is one block, its header, annotated `Parent Loop <row loop> Depth=3`)"""
    m = re.search(r"^%s\w*:.*?^\s*s_endpgm" % kernel, text, re.M | re.S)
    assert m, "kernel not in the listing"
    blocks = re.split(r"^(?=\.LBB\d+_\d+:)", m.group(0), flags=re.M)
    out = {}
    for b in blocks:
        lab = re.match(r"\.L(BB\d+_\d+):", b)
        head = "\n".join(b.splitlines()[:16])
        if not lab or not re.search(r"Loop Header: Depth=4", head):
            continue
        parents = re.findall(r"Parent Loop (BB\d+_\d+) Depth=3", head)
        if parents and parents[0] in row_headers:
            lines = [ln.split(";")[0].strip() for ln in b.splitlines()[1:]]
            back = [i for i, ln in enumerate(lines) if re.match(r"s_cbranch_\w+\s+\.L%s$" % lab.group(1), ln)]
            assert back, "no back edge in %s" % lab.group(1)
            out[lab.group(1)] = [ln for ln in lines[: back[0] + 1] if ln]
    return out


def test_one_pass_row_cycles(loops):
    assert loops[1][2] <= CAP_ONE_PASS, loops[1]


def test_two_pass_row_cycles(loops):
    assert loops[2][2] <= CAP_TWO_PASS, loops[2]


def test_snake_loops_form_no_address_by_shift(listing, loops):
    snakes = snake_loop_bodies(listing, {loops[1][0], loops[2][0]})
    print({h: len(b) for h, b in snakes.items()})
    assert len(snakes) == 3, "one snake loop in the one-pass row and two in the two-pass row, found %s" % sorted(snakes)
    for h, body in snakes.items():
        assert any(ln.startswith("v_alignbit_b32") for ln in body), "%s is not a snake loop: %s" % (h, body)
        bad = [ln for ln in body if ln.startswith("v_lshl_add_u32")]
        assert not bad, "%s: %s" % (h, bad)
