"""dw_extend2's ring of d-rows at linear LDS addresses, read in the compiler's gfx950 listing (no GPU needed, only hipcc; the file is compiled
once).

Ring positions used to be byte counters that every access wrapped into the half's 2 KB ring with one v_and_or_b32 (and an add in front
of it for the right neighbour, the second pass and its store): four such instructions in the one-pass row, ten in the two-pass row, 14 and
32 of their 134 / 224 listed issue cycles.  Positions are LDS addresses now and a row never straddles the ring's end (the rare row that
would is relocated to the ring's origin, outside the two fast loops), so the accesses take the position register as it is, the right
neighbour and pass 2 by the instruction's immediate offset; what the loops pay for it is one vector compare per row (4 cycles) and two
scalar instructions (profiles/dw_ring_linear.md).

The two fast d-row loops are found the way test_dw_row_cycles_cpu.fast_row_loops finds them and priced with its cost table:

* 134 - 14 + 4 = 124 cycles for the one-pass row, 224 - 32 + 4 = 196 for the two-pass row, which is what the compiler lists: the caps;
* the v_and_or_b32 left are those of the snake windows (match16_le2): two per snake loop;
* every ds_read_i16 / ds_write_b16 takes an address register whose last writer in the loop is a move or an add — no masking form —, and,
  in front of the row maximum (behind it sits the one store that forms its own address, the entry behind a row that fills all 32 lanes),
  a move is a copy of a register last written by an add: the position's advance, or the band update's rlin + step;
* resources of both instances: 64 VGPRs, eight waves per SIMD, 19 456 bytes of LDS, no scratch access at loop depth 2 or more; scratch at
  most 48 bytes per lane for dw_extend2<false> (test_dw_resources_cpu's bound) and at most 88 for dw_extend2<true>, which is what it had
  before positions became addresses."""
import os
import re
import subprocess

import pytest

import test_dw_row_cycles_cpu as R
import test_dw_row_scalar_cpu as S

CAP_ONE_PASS, CAP_TWO_PASS = 124, 196
AND_OR_ONE_PASS, AND_OR_TWO_PASS = 2, 4
SCRATCH_CAP = {"pw": 48, "cns": 88}
PLAIN = ("v_mov_b32", "v_add_u32", "v_add3_u32", "v_lshl_add_u32", "v_add_lshl_u32", "v_sub_u32", "v_subrev_u32")

pytestmark = pytest.mark.skipif(not os.path.exists(R.HIPCC), reason="no hipcc")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    out = tmp_path_factory.mktemp("dwring") / "dw_extend2.s"
    r = subprocess.run([R.HIPCC] + R._hipflags() + ["-x", "hip", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                    os.path.join("mecat_amd", "csrc", "dw_extend2.hip"), "-o", str(out)],
                       cwd=R.ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr, open(out).read()


@pytest.fixture(scope="module", params=sorted(S.KERNELS))
def inst(request, compiled):
    """(name, mangled prefix, {1: (header, VALU, cycles), 2: ...}, {1: instructions of the one-pass loop, 2: of the two-pass loop})"""
    kernel = S.KERNELS[request.param]
    found = R.fast_row_loops(compiled[1], kernel)
    assert sorted(found) == [1, 2], "expected the one-pass and the two-pass loop, found %s" % found
    rows = {n: S.loop_instructions(compiled[1], found[n][0], kernel) for n in (1, 2)}
    print(request.param, found)
    return request.param, kernel, found, rows


def test_row_cycles(compiled):
    """dw_extend2<false>, which the caps are derived for (dw_extend2<true> adds the row log to every row)"""
    found = R.fast_row_loops(compiled[1], S.KERNELS["pw"])
    print(found)
    assert sorted(found) == [1, 2], "expected the one-pass and the two-pass loop, found %s" % found
    assert found[1][2] <= CAP_ONE_PASS, found[1]
    assert found[2][2] <= CAP_TWO_PASS, found[2]


def test_no_mask_per_ring_access(inst):
    name, _, _, rows = inst
    extra = 1 if name == "cns" else 0          # (dw_extend2<true>: one more in the row log's address, as before)
    for n, cap in ((1, AND_OR_ONE_PASS), (2, AND_OR_TWO_PASS)):
        got = [a for op, a in rows[n] if op == "v_and_or_b32"]
        print(name, n, got)
        assert len(got) <= cap + extra, (n, got)


def _last_writer(ins, i, reg):
    """index of the last vector instruction in front of ins[i], going round the loop, that writes `reg`"""
    for j in list(range(i - 1, -1, -1)) + list(range(len(ins) - 1, i, -1)):
        op, args = ins[j]
        if op.startswith("v_") and args.split(",")[0].strip() == reg:
            return j
    return None


def test_ring_accesses_take_positions_as_they_are(inst):
    name, _, _, rows = inst
    for n in (1, 2):
        ins = rows[n]
        top = [i for i, (op, _) in enumerate(ins) if op.startswith("v_permlane16_swap")][0]
        acc = [i for i, (op, _) in enumerate(ins) if op in ("ds_read_i16", "ds_write_b16")]
        assert len(acc) >= 3 * n, "loop %d holds no ring accesses: %s" % (n, acc)
        for i in acc:
            op, args = ins[i]
            reg = args.split(",")[1 if op == "ds_read_i16" else 0].strip().split()[0]
            j = _last_writer(ins, i, reg)
            if j is None:
                continue                       # not written in the loop at all
            wop, wargs = ins[j]
            assert wop.split("_e")[0] in PLAIN, "%s loop %d: %s %s takes an address made by %s %s" % (name, n, op, args, wop, wargs)
            if i > top:
                continue                       # behind the row maximum: the `full` store, the one access that forms its own address
            if wop.startswith("v_mov_b32"):    # a copy of a position (the row that ran last = where this row starts)
                reg = wargs.split(",")[1].strip()
                j = _last_writer(ins, j, reg)
                assert j is not None and ins[j][0].split("_e")[0] in PLAIN[1:], "%s loop %d: %s %s: a copy of %s" % (name, n, op, args, ins[j] if j else None)


def _figures(remarks, kernel):
    fig, on = {}, False
    for ln in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1).startswith("Function Name:"):
            on = kernel in m.group(1)
        elif on and ":" in m.group(1):
            k, v = m.group(1).rsplit(":", 1)
            fig[k.strip()] = v.strip()
    return fig


def test_resources(inst, compiled):
    name, kernel, _, _ = inst
    fig = _figures(compiled[0], kernel)
    print(name, fig)
    assert int(fig["VGPRs"]) == 64
    assert int(fig["AGPRs"]) == 0
    assert int(fig["Occupancy [waves/SIMD]"]) == 8
    assert int(fig["LDS Size [bytes/block]"]) == 19456
    assert int(fig["ScratchSize [bytes/lane]"]) <= SCRATCH_CAP[name]
    assert fig["Dynamic Stack"] == "False"
    # no scratch instruction in a block of loop depth 2 or more (test_dw_resources_cpu's walk over the listing's loop annotations)
    m = re.search(r"^%s\w*:.*?^\s*s_endpgm" % kernel, compiled[1], re.M | re.S)
    assert m, "kernel not in the listing"
    depth, deep, bad = 0, 0, []
    for ln in m.group(0).splitlines():
        if re.match(r"^\.LBB\d+_\d+:", ln) or re.match(r"^; %bb\.\d+:", ln):
            d = re.search(r"Depth=(\d+)", ln)
            depth = int(d.group(1)) if d else 0
            deep = max(deep, depth)
        elif re.search(r"This (Inner )?Loop Header: Depth=(\d+)", ln):
            depth = int(re.search(r"Loop Header: Depth=(\d+)", ln).group(1))
            deep = max(deep, depth)
        elif ln.split(";")[0].strip().startswith("scratch_") and depth >= 2:
            bad.append(ln.strip())
    assert deep >= 3, "no loop annotations in the listing"
    assert not bad, bad
