"""CPU tier: the registers of vk_score_local_kernel (vk_score_m9f.hip, DESIGN 11.12: the flat-tailed bound pass over the compact 6-bit
shadow under local alignment, with the straight-line DP for groups of full 32-token slices), from the compiler's resource remarks
alone -- nothing is run.  tools/kernel_regs.py compiles the unit for gfx950.  Every instantiation allocates at most 104 registers
(four waves per SIMD, the budget of vk_score_m9t.hip) and has no scratch, and the instantiations are exactly the ones the unit's
launcher dispatches to: one per query length 1 .. 16, over a strip of LT = 4 * ceil(LQ / 4) columns.  Skipped where hipcc is missing."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"   # the compiler tools/kernel_regs.py calls
UNIT = os.path.join(ROOT, "vectorian_amd", "csrc", "vk_score_m9f.hip")
LINE = re.compile(r"vk_score_local_kernel<(\d+), (\d+)>.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)")
DISPATCHED = [((lq + 3) // 4 * 4, lq) for lq in range(1, 17)]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: nothing to compile with")


@pytest.fixture(scope="module")
def report():
	"""(the tool's text, {(lt, lq): (vgpr, agpr, allocated, scratch)})"""
	p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), UNIT], cwd=ROOT, capture_output=True, text=True)
	assert p.returncode == 0, p.stderr
	print(p.stdout)
	return p.stdout, {(int(m.group(1)), int(m.group(2))): tuple(int(x) for x in m.groups()[2:]) for m in LINE.finditer(p.stdout)}


def test_the_unit_holds_the_dispatched_forms_and_no_other_kernel(report):
	text, rows = report
	assert sorted(rows) == DISPATCHED, sorted(rows)
	assert len([line for line in text.splitlines() if " vgpr " in line]) == len(DISPATCHED), text   # ... and nothing beside them


def test_the_launcher_names_every_form_once():
	"""the launcher's cases are the lengths 1 .. 16, each on <4 * ceil(LQ / 4), LQ> (the macro of the unit's switch)"""
	src = open(UNIT).read()
	assert "vk_score_local_kernel<(LQ + 3) / 4 * 4, LQ>" in src
	assert [int(x) for x in re.findall(r"VK_M9F_CASE\((\d+)\)", src)] == list(range(1, 17))


def test_every_form_fits_104_registers_without_scratch(report):
	_, rows = report
	assert rows
	for (lt, lq), (vgpr, agpr, alloc, scratch) in sorted(rows.items()):
		assert alloc == (vgpr + agpr + 7) // 8 * 8
		assert scratch == 0, (lt, lq, scratch)
		assert alloc <= 104, (lt, lq, vgpr, agpr, alloc)
