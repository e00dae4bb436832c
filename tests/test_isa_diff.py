"""tools/isa_diff.py on two synthetic assembly snippets: kernels that are equal up to
label numbers, comments and the file they sit in compare as the same; one changed
operand, or one changed descriptor line, is a difference."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import isa_diff  # noqa: E402

KERNEL = """\
\t.text
\t.globl\t_Z3k_aPm
_Z3k_aPm:                               ; @_Z3k_aPm
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v0, {imm}                 ; {comment}
.LBB{n}_1:                                ; =>This Inner Loop Header: Depth=1
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dword v0, v0, s[0:1]
\ts_cbranch_scc1 .LBB{n}_1
\ts_endpgm
.Lfunc_end{n}:
\t.size\t_Z3k_aPm, .Lfunc_end{n}-_Z3k_aPm
\t.amdhsa_kernel _Z3k_aPm
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 6
\t.end_amdhsa_kernel
"""
OTHER = KERNEL.replace("_Z3k_aPm", "_Z3k_bPm")


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_equal_up_to_labels_comments_and_files(tmp_path):
    old = write(tmp_path, "old.s", OTHER.format(imm=7, comment="x", n=3, vgpr=1) + KERNEL.format(imm=7, comment="x", n=18, vgpr=1))
    new1 = write(tmp_path, "new1.s", KERNEL.format(imm=7, comment="moved here", n=0, vgpr=1))
    new2 = write(tmp_path, "new2.s", OTHER.format(imm=7, comment="y", n=5, vgpr=1))
    assert isa_diff.compare([old, "-"], [new1, new2]) == ([], [], [])


def test_changed_operand_descriptor_and_kernel_set(tmp_path):
    old = write(tmp_path, "old.s", KERNEL.format(imm=7, comment="x", n=1, vgpr=1))
    op = write(tmp_path, "op.s", KERNEL.format(imm=8, comment="x", n=1, vgpr=1))
    missing, added, differing = isa_diff.compare([old], [op])
    assert not missing and not added and [n for n, _ in differing] == ["_Z3k_aPm"]
    assert differing[0][1].startswith("text")
    desc = write(tmp_path, "desc.s", KERNEL.format(imm=7, comment="x", n=1, vgpr=2))
    _, _, differing = isa_diff.compare([old], [desc])
    assert [n for n, _ in differing] == ["_Z3k_aPm"] and differing[0][1].startswith("descriptor")
    other = write(tmp_path, "other.s", OTHER.format(imm=7, comment="x", n=1, vgpr=1))
    assert isa_diff.compare([old], [other]) == (["_Z3k_aPm"], ["_Z3k_bPm"], [])
