"""dw_extend2's one-pass row without its `full` test, read in the compiler's gfx950 listing (no GPU needed, only hipcc; the file is compiled once).

The one-pass loop tested on every row whether a half has exactly 32 slots (s_or_b32, s_bitcmp0_b32 and a branch), to store the entry
behind such a row, which no idle lane of that half stores.  Every lane now stores that entry one slot to its right in front of its own
store — ds_write_b16 … offset:2, then ds_write_b16 at the position itself —, so slots 1 .. 31 end up as they did and slot 32 holds the
entry.  That is two separate stores in program order: merged into one ds_write_b32 (through a v_perm_b32), lanes i and i + 1 would write
slot i + 1 in the same instruction.  So, for both instances of the kernel:

* the one-pass loop lists at most 31 scalar instructions (it had 33; counted as test_dw_row_scalar_cpu counts them);
* it holds no s_bitcmp0_b32, exactly two ds_write_b16, one of them with offset:2 and that one first, no ds_write_b32 and no v_perm_b32;
* the two-pass loop keeps its caps: 47 scalar instructions, and 196 cycles for dw_extend2<false>
  (profiles/dw_row_exits.md)."""
import os

import pytest

import test_dw_ring_linear_cpu as L
import test_dw_row_cycles_cpu as R
import test_dw_row_scalar_cpu as S
from test_dw_ring_linear_cpu import compiled, inst  # noqa: F401  (the module's fixtures: one compilation, both instances)

CAP_ONE_PASS_SCALAR = 31

pytestmark = pytest.mark.skipif(not os.path.exists(R.HIPCC), reason="no hipcc")


def test_one_pass_row_scalar_count(inst):
    name, _, _, rows = inst
    n = S.salu(rows[1])
    print(name, n)
    assert n <= CAP_ONE_PASS_SCALAR, [i for i in rows[1] if i[0].startswith("s_")]


def test_one_pass_row_has_no_full_test(inst):
    name, _, _, rows = inst
    ops = [op for op, _ in rows[1]]
    assert "s_bitcmp0_b32" not in ops, name


def test_one_pass_row_stores(inst):
    name, _, _, rows = inst
    st = [args for op, args in rows[1] if op == "ds_write_b16"]
    print(name, st)
    assert len(st) == 2, st
    assert "offset:2" in st[0].split() and "offset" not in st[1], "the entry behind the row is stored first, one slot to the right: %s" % st
    assert st[0].split(",")[0].strip() == st[1].split(",")[0].strip(), "both stores take the row's position: %s" % st
    ops = [op for op, _ in rows[1]]
    assert "ds_write_b32" not in ops, "the two stores of a lane were merged"
    assert not [op for op in ops if op.startswith("v_perm_b32")]


def test_two_pass_row_keeps_its_caps(inst):
    name, _, found, rows = inst
    n = S.salu(rows[2])
    print(name, n, found[2])
    assert n <= S.CAP_TWO_PASS
    if name == "pw":
        assert found[2][2] <= L.CAP_TWO_PASS, found[2]

