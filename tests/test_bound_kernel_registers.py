"""CPU tier: the register budget of the 6-bit bound kernels, from the compiler's resource remarks alone -- nothing is run.
tools/kernel_regs.py compiles vk_score_m8.hip (linear, affine and general gaps over the 32-row history) and vk_score_m8w.hip (the
64-row history) for gfx950 and prints one line per kernel.  Every form must allocate at most 120 registers (VGPRs + AGPRs, in the
allocation's steps of 8) and no scratch: four waves of it per SIMD then leave 32 registers or more, three leave 152, and a wave of
the rounds' exact kernel finds room beside the pass.  The figures move with the toolchain (two empty asm statements keep the compiler
from hoisting loop invariants into the kernels' lifetime): this is the check that DESIGN 11.8 asked to be made by hand at every ROCm
upgrade.  Skipped where hipcc is missing."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"   # the compiler tools/kernel_regs.py calls
BUDGET = 120
LINE = re.compile(r"vk_score_kernel<8, 3, false, (\d+), (\d+)>.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: nothing to compile with")


@pytest.fixture(scope="module")
def reports():
	"""{unit: {(gap, lt): (vgpr, agpr, allocated, scratch)}}, both units compiled side by side"""
	units = ("vk_score_m8.hip", "vk_score_m8w.hip")
	procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), os.path.join(ROOT, "vectorian_amd", "csrc", u)],
		cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for u in units]
	out = {}
	for u, p in zip(units, procs):
		text, err = p.communicate()
		assert p.returncode == 0, err
		print(text)
		out[u] = {(int(m[1]), int(m[2])): tuple(int(x) for x in m.groups()[2:]) for m in LINE.finditer(text)}
	return out


@pytest.mark.parametrize("unit,gaps", (("vk_score_m8.hip", (0, 1, 3)), ("vk_score_m8w.hip", (6,))))
def test_every_form_keeps_the_budget_without_scratch(reports, unit, gaps):
	rows = reports[unit]
	assert sorted(rows) == [(g, lt) for g in gaps for lt in (4, 8, 12, 16)], sorted(rows)
	for (gap, lt), (vgpr, agpr, alloc, scratch) in sorted(rows.items()):
		assert alloc == (vgpr + agpr + 7) // 8 * 8
		assert alloc <= BUDGET, (unit, gap, lt, vgpr, agpr, alloc)
		assert scratch == 0, (unit, gap, lt, scratch)
