"""Issue cycles of dw_extend2<false>'s two fast d-row loops, priced from the compiler's gfx950 listing (no GPU needed, only hipcc).

The kernel is VALU-issue bound, so the vector instructions of a row priced by their issue class are its time.  The loops are found the way
`tools/isa_mix.py --row-loops` finds row loops, one level further down: the depth-3 loops that contain the half-wave row maximum
(v_permlane16_swap) — the one-pass loop has one snake loop nested in it, the two-pass loop two.  Their VALU instructions are priced with
`isa_mix.classify`: 2 cycles for the plain 32-bit add / sub / logic / mov / shift right, 4 for everything else.

Caps: the parent of the commit that added this test had 174 cycles per one-pass row and 280 per two-pass row.  Doubling by add, the row count
on the scalar unit, the cut without saturation and positions in doubled units were derived to 160 / 262 (profiles/dw_row_trims.md); the caps
leave two cycles for scheduling differences.  The band update's values handed over packed by the scalar unit took the loops further, to
146 / 248; the caps stay where the derivation put them."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_mix  # noqa: E402

HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNEL = "_Z10dw_extend2ILb0E"
CAP_ONE_PASS, CAP_TWO_PASS = 162, 264

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def _hipflags():
    """HIPFLAGS of the Makefile, its variables filled in"""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, re.M)}
    flags = var["HIPFLAGS"]
    for _ in range(4):
        flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], flags)
    return flags.split()


def fast_row_loops(text, kernel=KERNEL):
    """{number of snake loops: (header label, VALU instructions, issue cycles)} of the depth-3 loops of `kernel` that hold the half-wave
    maximum; a snake loop's body counts once (one snake step per pass: what 99.5 % of the passes run)"""
    m = re.search(r"^%s\w*:.*?^\s*s_endpgm" % kernel, text, re.M | re.S)
    assert m, "kernel not in the listing"
    blocks = []
    for ln in m.group(0).splitlines():
        lab = re.match(r"^\.L(BB\d+_\d+):", ln)
        if lab or re.match(r"^; %bb\.\d+:", ln) or not blocks:
            blocks.append({"label": lab.group(1) if lab else None, "lines": []})
        blocks[-1]["lines"].append(ln)
    parent, depth = {}, {}
    for b in blocks:
        head = "\n".join(b["lines"][:16])
        mh = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", head)
        mi = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", b["lines"][0])
        if mh and b["label"]:
            b["loop"] = b["label"]
            depth[b["label"]] = int(mh.group(1))
            ps = [(int(d), h) for h, d in re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", head)]
            parent[b["label"]] = max(ps)[1] if ps else None
        else:
            b["loop"] = mi.group(1) if mi else None

    def chain(h):
        out = []
        while h:
            out.append(h)
            h = parent.get(h)
        return out

    found = {}
    for h in [h for h, d in depth.items() if d == 3]:
        mine = [b for b in blocks if b["loop"] and h in chain(b["loop"])]
        if not any("v_permlane16_swap" in ln for b in mine for ln in b["lines"]):
            continue
        snakes = sum(1 for c, p in parent.items() if p == h)
        # Blocks that a forward conditional branch inside the loop jumps over are left out: the row is priced along its common path
        # (the one-pass loop has one such block, the store of the entry behind a row that fills all 32 lanes of a half).
        skipped = set()
        for i, blk in enumerate(mine):
            br = [re.match(r"\s*s_cbranch_\w+\s+\.L(BB\d+_\d+)", ln) for ln in blk["lines"]]
            for mb in [x for x in br if x]:
                later = [j for j in range(i + 1, len(mine)) if mine[j]["label"] == mb.group(1)]
                if later and all(mine[j]["loop"] == blk["loop"] for j in range(i, later[0] + 1)):
                    skipped.update(range(i + 1, later[0]))
        valu = cycles = 0
        for b in [blk for i, blk in enumerate(mine) if i not in skipped]:
            for ln in b["lines"]:
                s = ln.split(";")[0].strip()
                mo = re.match(r"([a-z_0-9]+)\s*(.*)", s)
                if not s or s.endswith(":") or s.startswith(".") or not mo:
                    continue
                c = isa_mix.classify(mo.group(1), mo.group(2))
                if c in ("valu2", "valu4"):
                    valu += 1
                    cycles += 2 if c == "valu2" else 4
        assert snakes not in found, "two row loops with %d snake loops" % snakes
        found[snakes] = (h, valu, cycles)
    return found


@pytest.fixture(scope="module")
def loops(tmp_path_factory):
    out = tmp_path_factory.mktemp("dwcyc") / "dw_extend2.s"
    r = subprocess.run([HIPCC] + _hipflags() + ["-x", "hip", "--cuda-device-only", "-S", os.path.join("mecat_amd", "csrc", "dw_extend2.hip"),
                                                "-o", str(out)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = fast_row_loops(open(out).read())
    print(found)
    assert sorted(found) == [1, 2], "expected the one-pass and the two-pass loop, found %s" % found
    return found


def test_one_pass_row_cycles(loops):
    assert loops[1][2] <= CAP_ONE_PASS, loops[1]


def test_two_pass_row_cycles(loops):
    assert loops[2][2] <= CAP_TWO_PASS, loops[2]
