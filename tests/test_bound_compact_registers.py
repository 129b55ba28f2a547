"""CPU tier: the registers of the bound kernels over the compact 6-bit shadow (MODE 9), from the compiler's resource
remarks alone -- nothing is run.  tools/kernel_regs.py compiles vk_score_m9.hip (linear, affine and general gaps over the 32-row
history), vk_score_m9t.hip (the flat-tailed forms: GAP 8, the 32-row history, GAP 9, the 64-row one) and vk_score_m9w.hip (general gaps
over the 64-row history) for gfx950.  No form may use scratch; the 32-row forms, which take two tiles per trip, allocate at most 104
registers (four waves per SIMD, as MODE 8's); the 64-row forms at most 120.  Skipped where hipcc is missing."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"   # the compiler tools/kernel_regs.py calls
LINE = re.compile(r"vk_score_kernel<(\d+), (\d+), false, (\d+), (\d+)>.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)")
LTS = (4, 8, 12, 16)
UNITS = {"vk_score_m9.hip": (0, 1, 3), "vk_score_m9t.hip": (8, 9), "vk_score_m9w.hip": (6,)}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: nothing to compile with")


@pytest.fixture(scope="module")
def reports():
	"""{unit: {(mode, steps, gap, lt): (vgpr, agpr, allocated, scratch)}}, the units compiled side by side"""
	procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), os.path.join(ROOT, "vectorian_amd", "csrc", u)],
		cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for u in UNITS]
	out = {}
	for u, p in zip(UNITS, procs):
		text, err = p.communicate()
		assert p.returncode == 0, err
		print(text)
		out[u] = {tuple(int(x) for x in m.groups()[:4]): tuple(int(x) for x in m.groups()[4:]) for m in LINE.finditer(text)}
	return out


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_compact_forms_keep_their_allocations_without_scratch(reports, unit):
	rows = reports[unit]
	assert sorted(rows) == [(9, 3, gap, lt) for gap in UNITS[unit] for lt in LTS], sorted(rows)
	for (_, _, gap, lt), (vgpr, agpr, alloc, scratch) in sorted(rows.items()):
		assert alloc == (vgpr + agpr + 7) // 8 * 8
		assert scratch == 0, (gap, lt, scratch)
		assert alloc <= (120 if gap in (6, 9) else 104), (gap, lt, vgpr, agpr, alloc)
