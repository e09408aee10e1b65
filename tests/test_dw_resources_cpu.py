"""dw_extend2<false>'s resource figures as the compiler reports them for gfx950 (no GPU needed, only hipcc): the kernel runs eight waves
per SIMD on 64 VGPRs and eight workgroups per CU on 19 456 bytes of LDS each; what spills goes to at most 48 bytes of scratch per lane,
none of it touched inside a d-row loop.  Code around the row loops (block set-up, traceback, accounting) must not push it off that."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNEL = "_Z10dw_extend2ILb0E"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def _hipflags():
    """HIPFLAGS of the Makefile, its variables filled in"""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, re.M)}
    flags = var["HIPFLAGS"]
    for _ in range(4):
        flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], flags)
    return flags.split()


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    out = tmp_path_factory.mktemp("dwres") / "align.s"
    r = subprocess.run([HIPCC] + _hipflags() + ["-x", "hip", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                os.path.join("mecat_amd", "csrc", "dw_extend2.hip"), "-o", str(out)],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr, open(out).read()


def _figures(remarks):
    """{name: value} of the remark lines that follow the kernel's `Function Name`"""
    fig, on = {}, False
    for ln in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1).startswith("Function Name:"):
            on = KERNEL in m.group(1)
        elif on and ":" in m.group(1):
            k, v = m.group(1).rsplit(":", 1)
            fig[k.strip()] = v.strip()
    return fig


def test_dw_extend2_resource_usage(compiled):
    fig = _figures(compiled[0])
    print(fig)
    assert int(fig["VGPRs"]) == 64
    assert int(fig["AGPRs"]) == 0
    assert int(fig["Occupancy [waves/SIMD]"]) == 8
    assert int(fig["LDS Size [bytes/block]"]) == 19456
    assert int(fig["ScratchSize [bytes/lane]"]) <= 48
    assert fig["Dynamic Stack"] == "False"


def test_dw_extend2_no_scratch_in_row_loops(compiled):
    """the listing's loop annotations: no scratch instruction in a basic block of loop depth 2 or more (the row loops and the snake
    loops inside them; depth 1 is the per-block code of the outer loop)"""
    text = compiled[1]
    m = re.search(r"^%s\w*:.*?^\s*s_endpgm" % KERNEL, text, re.M | re.S)
    assert m, "kernel not in the listing"
    depth, deep, bad = 0, 0, []
    for ln in m.group(0).splitlines():
        if re.match(r"^\.LBB\d+_\d+:", ln) or re.match(r"^; %bb\.\d+:", ln):
            d = re.search(r"Depth=(\d+)", ln)
            depth = int(d.group(1)) if d else 0
            deep = max(deep, depth)
        elif re.search(r"This (Inner )?Loop Header: Depth=(\d+)", ln):      # a loop header's own depth follows its parents' lines
            depth = int(re.search(r"Loop Header: Depth=(\d+)", ln).group(1))
            deep = max(deep, depth)
        elif ln.split(";")[0].strip().startswith("scratch_") and depth >= 2:
            bad.append(ln.strip())
    assert deep >= 3, "no loop annotations in the listing"          # outer loop, row loop, snake loop
    assert not bad, bad
