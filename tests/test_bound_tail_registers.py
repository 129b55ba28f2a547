"""CPU tier: the registers of the flat-tailed bound kernels, from the compiler's resource remarks alone -- nothing is run.
tools/kernel_regs.py compiles vk_score_m8t.hip (MODE 8: GAP 8, the 32-row history, and GAP 9, the 64-row history) and vk_score_m7t.hip
(MODE 7 at five and at twelve K-steps, both histories) for gfx950.  No form may use scratch; the 32-row forms of MODE 8 allocate at
most 104 registers (four waves per SIMD, as the forms they stand in for), its 64-row forms at most 120.  The MODE 7 forms are printed
and recorded, not bounded: LDS, not registers, limits them (vk_score_m7w.hip).  Skipped where hipcc is missing."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"   # the compiler tools/kernel_regs.py calls
LINE = re.compile(r"vk_score_kernel<(\d+), (\d+), false, (\d+), (\d+)>.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)")
LTS = (4, 8, 12, 16)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: nothing to compile with")


@pytest.fixture(scope="module")
def reports():
	"""{unit: {(mode, steps, gap, lt): (vgpr, agpr, allocated, scratch)}}, both units compiled side by side"""
	units = ("vk_score_m8t.hip", "vk_score_m7t.hip")
	procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), os.path.join(ROOT, "vectorian_amd", "csrc", u)],
		cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for u in units]
	out = {}
	for u, p in zip(units, procs):
		text, err = p.communicate()
		assert p.returncode == 0, err
		print(text)
		out[u] = {tuple(int(x) for x in m.groups()[:4]): tuple(int(x) for x in m.groups()[4:]) for m in LINE.finditer(text)}
	return out


def test_mode8_forms_keep_their_allocations_without_scratch(reports):
	rows = reports["vk_score_m8t.hip"]
	assert sorted(rows) == [(8, 3, gap, lt) for gap in (8, 9) for lt in LTS], sorted(rows)
	for (_, _, gap, lt), (vgpr, agpr, alloc, scratch) in sorted(rows.items()):
		assert alloc == (vgpr + agpr + 7) // 8 * 8
		assert scratch == 0, (gap, lt, scratch)
		assert alloc <= (104 if gap == 8 else 120), (gap, lt, vgpr, agpr, alloc)


def test_mode7_forms_are_recorded_without_scratch(reports, record_property):
	rows = reports["vk_score_m7t.hip"]
	assert sorted(rows) == [(7, steps, gap, lt) for steps in (5, 12) for gap in (8, 9) for lt in LTS], sorted(rows)
	for key, (vgpr, agpr, alloc, scratch) in sorted(rows.items()):
		record_property("vk_score_kernel<%d, %d, false, %d, %d>" % key, "vgpr %d agpr %d alloc %d scratch %d" % (vgpr, agpr, alloc, scratch))
		assert alloc == (vgpr + agpr + 7) // 8 * 8
		assert scratch == 0, (key, scratch)
