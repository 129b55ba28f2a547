"""CPU tier: the table kernel of the vector similarities beside the cosine (vk_source_table_kernel, vk_pack.hip), from the
compiler's resource remarks alone -- nothing is run.  tools/kernel_regs.py compiles vk_pack.hip for gfx950 and prints one line per
kernel: each of the four forms (p = 1, p = 2, general p, sqrt-cosine) keeps its sixteen double partial sums in registers and reports
0 bytes of scratch -- an array indexed by a run-time value would move them to memory.  Skipped where hipcc is missing."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"   # the compiler tools/kernel_regs.py calls
LINE = re.compile(r"vk_source_table_kernel<(\d+)>.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: nothing to compile with")


def test_every_form_of_the_source_table_kernel_is_free_of_scratch():
	p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), os.path.join(ROOT, "vectorian_amd", "csrc", "vk_pack.hip")],
		cwd=ROOT, capture_output=True, text=True)
	assert p.returncode == 0, p.stderr
	rows = {int(m[1]): tuple(int(x) for x in m.groups()[1:]) for m in LINE.finditer(p.stdout)}
	print(rows)
	assert sorted(rows) == [0, 1, 2, 3], p.stdout
	for form, (vgpr, agpr, alloc, scratch) in rows.items():
		assert scratch == 0, (form, vgpr, agpr, scratch)
		assert alloc <= 128, (form, alloc)   # four waves per SIMD and more: the kernel is bound by its adds, not by occupancy
