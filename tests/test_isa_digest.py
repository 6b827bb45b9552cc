"""tools/isa_digest.py --per-kernel on two small synthetic listings (no compiler, no device): the
per-function hash does not depend on where the function stands in its unit or on how the listing
is laid out, and it does depend on every instruction and on the kernel descriptor."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_digest", os.path.join(ROOT, "tools", "isa_digest.py"))
isa_digest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_digest)


def function(sym, index, op="v_add_f32_e32 v0, v0, v1", vgprs=8, pad=" "):
    """One kernel as the compiler lays it out: `index` is its position in the unit (it numbers the
    block labels and .Lfunc_end), `pad` the blanks in front of the trailing comments."""
    return f"""\t.protected\t{sym}
\t.globl\t{sym}
\t.p2align\t8
\t.type\t{sym},@function
{sym}:{pad}; @{sym}
; %bb.0:
\ts_load_dword s2, s[0:1], 0x0
\ts_cbranch_scc1 .LBB{index}_2{pad}; taken at the end
.LBB{index}_1:{pad}; %loop
\t{op}
\ts_cbranch_vccnz .LBB{index}_1
.LBB{index}_2:
\ts_endpgm
.Lfunc_end{index}:
\t.size\t{sym}, .Lfunc_end{index}-{sym}
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {sym}
\t\t.amdhsa_next_free_vgpr {vgprs}
\t\t.amdhsa_next_free_sgpr 6
\t.end_amdhsa_kernel
\t.text
"""


def lines(listing):
    """the tool's output for one unit: a line per function, sorted by symbol"""
    return [f"{h}  unit.hip  {sym}" for sym, h in sorted(isa_digest.per_kernel(listing.encode()).items())]


HEAD = "\t.text\n\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n"
TAIL = "\t.type\t__hip_cuid_0123abcd,@object\n__hip_cuid_0123abcd:\n\t.byte\t0\n"


def test_order_block_indices_and_comment_alignment_do_not_matter():
    a = HEAD + function("_Z3fooPd", 0) + function("_Z3barPd", 1) + TAIL
    b = HEAD + function("_Z3barPd", 0, pad="      ") + function("_Z3fooPd", 1, pad="\t\t") + TAIL.replace("0123abcd", "99ff")
    assert len(lines(a)) == 2
    assert lines(a) == lines(b)


def test_one_instruction_changes_exactly_that_function():
    a = HEAD + function("_Z3fooPd", 0) + function("_Z3barPd", 1)
    b = HEAD + function("_Z3fooPd", 0) + function("_Z3barPd", 1, op="v_sub_f32_e32 v0, v0, v1")
    la, lb = lines(a), lines(b)
    changed = [x.split()[-1] for x, y in zip(la, lb) if x != y]
    assert [x.split()[-1] for x in la] == [x.split()[-1] for x in lb]
    assert changed == ["_Z3barPd"]


def test_one_descriptor_field_changes_exactly_that_function():
    a = HEAD + function("_Z3fooPd", 0) + function("_Z3barPd", 1)
    b = HEAD + function("_Z3fooPd", 0, vgprs=9) + function("_Z3barPd", 1)
    changed = [x.split()[-1] for x, y in zip(lines(a), lines(b)) if x != y]
    assert changed == ["_Z3fooPd"]
