"""CPU: tools/kernel_diff.py on four short listings written out here -- identical, one operand changed, one kernel missing, padding moved only."""
import importlib.util
import os

from tests import common

_spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(common.ROOT, "tools", "kernel_diff.py"))
kernel_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kernel_diff)

# two kernels as `llvm-objdump -d` prints them (the second with a backward branch: its operand is a relative offset) and their symbols as `llvm-objdump -t` does;
# the four bytes at 0x1110 lie behind the first kernel's size: padding
_PARENT = """
/tmp/a.co:\tfile format elf64-amdgpu

Disassembly of section .text:

0000000000001100 <_Z5firstPd>:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001100: C0060002 00000000
\tv_mov_b32_e32 v0, 0                                        // 000000001108: 7E000280
\ts_endpgm                                                   // 00000000110C: BF810000
\ts_nop 0                                                    // 000000001110: BF800000

0000000000001200 <_Z6secondPdi>:
\tv_add_u32_e32 v1, 1, v1                                    // 000000001200: 68020281
\ts_cbranch_scc1 65534                                       // 000000001204: BF85FFFE <_Z6secondPdi>
\ts_endpgm                                                   // 000000001208: BF810000
"""
_PARENT_SYMS = """
SYMBOL TABLE:
0000000000000040 l       *ABS*\t0000000000000000 _Z5firstPd.num_vgpr
0000000000001100 g     F .text\t0000000000000010 .protected _Z5firstPd
0000000000001200 g     F .text\t000000000000000c .protected _Z6secondPdi
0000000000000100 g     O .rodata\t0000000000000040 .protected _Z5firstPd.kd
"""
# the same two kernels in the other order, at other addresses, the first with more padding behind it
_MOVED = """
Disassembly of section .text:

0000000000002000 <_Z6secondPdi>:
\tv_add_u32_e32 v1, 1, v1                                    // 000000002000: 68020281
\ts_cbranch_scc1 65534                                       // 000000002004: BF85FFFE <_Z6secondPdi>
\ts_endpgm                                                   // 000000002008: BF810000

0000000000002100 <_Z5firstPd>:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000002100: C0060002 00000000
\tv_mov_b32_e32 v0, 0                                        // 000000002108: 7E000280
\ts_endpgm                                                   // 00000000210C: BF810000
\ts_nop 0                                                    // 000000002110: BF800000
\ts_nop 0                                                    // 000000002114: BF800000
\ts_nop 0                                                    // 000000002118: BF800000
"""
_MOVED_SYMS = """
SYMBOL TABLE:
0000000000002000 g     F .text\t000000000000000c .protected _Z6secondPdi
0000000000002100 g     F .text\t0000000000000010 .protected _Z5firstPd
"""


def _verdict(parent, new):
    same, diff, added, missing = kernel_diff.compare(parent, new)
    return (len(same), diff, added, missing, kernel_diff.accepted(same, diff, added, missing, len(parent)))


def test_kernel_diff_on_four_listings():
    parent = kernel_diff.kernels(_PARENT, _PARENT_SYMS)
    assert parent == {"_Z5firstPd": ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v0, 0", "s_endpgm"],
                      "_Z6secondPdi": ["v_add_u32_e32 v1, 1, v1", "s_cbranch_scc1 65534", "s_endpgm"]}
    # identical
    assert _verdict(parent, kernel_diff.kernels(_PARENT, _PARENT_SYMS)) == (2, [], [], [], True)
    # one operand changed (a branch offset: it takes part)
    changed = kernel_diff.kernels(_PARENT.replace("s_cbranch_scc1 65534", "s_cbranch_scc1 65533"), _PARENT_SYMS)
    assert _verdict(parent, changed) == (1, ["_Z6secondPdi"], [], [], False)
    # one kernel missing -- and, seen from the other side, one new
    cut = _PARENT[:_PARENT.index("0000000000001200 <")]
    fewer = kernel_diff.kernels(cut, _PARENT_SYMS)
    assert _verdict(parent, fewer) == (1, [], [], ["_Z6secondPdi"], False)
    assert _verdict(fewer, parent) == (1, [], ["_Z6secondPdi"], [], False)
    # padding, addresses and symbol order moved, nothing else
    assert _verdict(parent, kernel_diff.kernels(_MOVED, _MOVED_SYMS)) == (2, [], [], [], True)
    # ... which only the symbol sizes tell from code: without them the longer padding is a difference
    assert _verdict(kernel_diff.kernels(_PARENT), kernel_diff.kernels(_MOVED)) == (1, ["_Z5firstPd"], [], [], False)
    # nothing parsed is not accepted
    assert _verdict({}, {}) == (0, [], [], [], False)
    lines, ok = kernel_diff.report({"lib.so: " + k: v for k, v in parent.items()}, {"lib.so: " + k: v for k, v in changed.items()})
    assert not ok and lines[0].endswith("1 identical, 1 different, 0 new, 0 missing") and "different: lib.so: _Z6secondPdi" in lines
