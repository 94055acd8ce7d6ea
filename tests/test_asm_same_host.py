"""tools/asm_same.py on two small listings written here: three functions each, compared function by function."""
import io
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import asm_same  # noqa: E402


def _function(name, body):
    return (f"\t.globl\t{name}\n\t.type\t{name},@function\n{name}:\n" + "".join(f"\t{i}\n" for i in body)
            + f".Lfunc_end_{name}:\n\t.size\t{name}, .Lfunc_end_{name}-{name}\n\t.section\t.rodata\n\t.amdhsa_kernel {name}\n")


def _listing(funcs, cuid):
    return ("\t.text\n" + "".join(_function(n, b) for n, b in funcs)
            + f"\t.type\t__hip_cuid_{cuid},@object\n__hip_cuid_{cuid}:\n\t.byte\t0\n\t.size\t__hip_cuid_{cuid}, 1\n")


F = [("_Z1av", ["s_load_dword s0, s[0:1], 0x0", "s_endpgm"]),
     ("_Z1bv", ["v_add_f32_e32 v0, v0, v1", "s_endpgm"]),
     ("_Z1cv", ["v_fma_f32 v0, v0, v1, v2", "s_endpgm"])]
CHANGED = [F[0], ("_Z1bv", ["v_sub_f32_e32 v0, v0, v1", "s_endpgm"]), F[2]]
EXTRA = F + [("_Z1dv", ["s_endpgm"])]


@pytest.mark.parametrize("b_funcs, status, lines", [
    (F, 0, ["3 / 3 functions: 0 differ, 0 added, 0 removed"]),
    (CHANGED, 1, ["differs _Z1bv", "3 / 3 functions: 1 differ, 0 added, 0 removed"]),
    (EXTRA, 1, ["added _Z1dv", "3 / 4 functions: 0 differ, 1 added, 0 removed"]),
    (F[:2], 1, ["removed _Z1cv", "3 / 2 functions: 0 differ, 0 added, 1 removed"]),
], ids=["same_but_cuid", "body_changed", "function_added", "function_removed"])
def test_asm_same(b_funcs, status, lines):
    out = io.StringIO()
    assert asm_same.compare(_listing(F, "1234abcd"), _listing(b_funcs, "9876fedc"), out) == status
    assert out.getvalue().splitlines() == lines


def test_functions_are_cut_at_type_and_size():
    fs = asm_same.functions(_listing(F, "1234abcd"))
    assert sorted(fs) == ["_Z1av", "_Z1bv", "_Z1cv"]
    assert "v_fma_f32" in fs["_Z1cv"] and "amdhsa_kernel" not in fs["_Z1cv"]


def _numbered(first, edit=lambda name, body: body):
    """The three functions with a loop each, as the `first`-th and following functions of a translation unit: the compiler
    puts a function's index into its local labels and into the comments that mention them."""
    funcs = []
    for k, (name, body) in enumerate(F):
        f = first + k
        funcs.append((name, edit(name, [f"s_cbranch_scc1 .LBB{f}_2", f".LBB{f}_1:", body[0],
                                        f"s_cbranch_vccnz .LBB{f}_1 ; in Loop: Header=BB{f}_1 Depth=1", f".LBB{f}_2:",
                                        f".Ltmp{3 * f}:", f"s_getpc_b64 s[0:1] ; .Ltmp{3 * f}", f".LBB{f}_3:", body[1],
                                        f".Lfunc_end{f}:"])))
    return funcs


def _b_changed(name, body):
    return [l.replace("v_add_f32_e32", "v_sub_f32_e32") for l in body]


def _b_retargeted(name, body):
    return [l.replace("s_cbranch_scc1 .LBB7_2", "s_cbranch_scc1 .LBB7_3") for l in body]


@pytest.mark.parametrize("b_funcs, status, lines", [
    (_numbered(6), 0, ["3 / 3 functions: 0 differ, 0 added, 0 removed"]),
    (_numbered(6, _b_changed), 1, ["differs _Z1bv", "3 / 3 functions: 1 differ, 0 added, 0 removed"]),
    (_numbered(6, _b_retargeted), 1, ["differs _Z1bv", "3 / 3 functions: 1 differ, 0 added, 0 removed"]),
], ids=["renumbered", "renumbered_instruction_changed", "renumbered_branch_retargeted"])
def test_asm_same_ignores_the_function_index_of_local_labels(b_funcs, status, lines):
    assert any(".LBB7_2" in l for l in dict(_numbered(6))["_Z1bv"])      # the function the edits aim at is number 7 there
    out = io.StringIO()
    assert asm_same.compare(_listing(_numbered(0), "1234abcd"), _listing(b_funcs, "9876fedc"), out) == status
    assert out.getvalue().splitlines() == lines
