"""tools/ir_fma_order.py on a miniature pair of IR files: the same sum of two products, its operands swapped in the second file."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IR = """define void @kern(double %a, double %b, double %c, double %d) {
  %m0 = fmul contract double %a, %b, !dbg !11
  %m1 = fmul contract double %c, %d, !dbg !12
  %s = fadd contract double OPERANDS, !dbg !13
  %m2 = fmul contract double %a, %d, !dbg !11
  %m3 = fmul contract double %c, %b, !dbg !12
  %t = fsub contract double %m2, %m3, !dbg !13
  ret void
}
!1 = distinct !DISubprogram(name: "dot2", scope: !0)
!2 = distinct !DISubprogram(name: "caller", scope: !0)
!10 = !DILocation(line: 40, column: 3, scope: !2)
!11 = !DILocation(line: 7, column: 10, scope: !1, inlinedAt: !10)
!12 = !DILocation(line: 7, column: 24, scope: !1, inlinedAt: !10)
!13 = !DILocation(line: 7, column: 19, scope: !1, inlinedAt: !10)
"""


def test_a_swapped_pair_of_products_is_reported(tmp_path):
    old, new = tmp_path / "old.ll", tmp_path / "new.ll"
    old.write_text(IR.replace("OPERANDS", "%m0, %m1"))
    new.write_text(IR.replace("OPERANDS", "%m1, %m0"))
    tool = os.path.join(ROOT, "tools", "ir_fma_order.py")
    same = subprocess.run([sys.executable, tool, "@kern", str(old), str(old)], capture_output=True, text=True, check=True).stdout
    assert "0 (operation, order, inlined-at chain) classes differ" in same and "old source 2" in same
    out = subprocess.run([sys.executable, tool, "@kern", str(old), str(new)], capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if ln.startswith("fadd")]
    assert len(lines) == 2 and all("dot2 < caller" in ln for ln in lines), out
    assert any("source" in ln and "old    1 new    0" in ln for ln in lines) and any("swapped" in ln and "old    0 new    1" in ln for ln in lines), out
    assert not [ln for ln in out.splitlines() if ln.startswith("fsub")]          # (the difference kept its order)
