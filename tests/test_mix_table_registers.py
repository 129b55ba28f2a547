"""CPU tier: the two kernels of the token similarity combinators (vk_canon_table_kernel, vk_table_mix_kernel, vk_mix.hip),
from the code object's resource metadata alone -- nothing is run.  tools/kernel_regs.py compiles vk_mix.hip for gfx950 and prints one
line per kernel.  vk_canon_table_kernel carries sim_canon16's sixteen double partial sums of a lane (four columns x four sums) and
its staging goes through LDS: 94 VGPRs, no scratch.  vk_table_mix_kernel holds four float4 loads and four double accumulators: 30
VGPRs, no scratch -- an operand array indexed by a run-time value would move the cells to memory.  Skipped where hipcc is missing."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"   # the compiler tools/kernel_regs.py calls
LINE = re.compile(r"(vk_canon_table_kernel|vk_table_mix_kernel)\(.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: nothing to compile with")


def test_the_mix_kernels_registers_and_no_scratch():
	p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), os.path.join(ROOT, "vectorian_amd", "csrc", "vk_mix.hip")],
		cwd=ROOT, capture_output=True, text=True)
	assert p.returncode == 0, p.stderr
	rows = {m[1]: tuple(int(x) for x in m.groups()[1:]) for m in LINE.finditer(p.stdout)}
	print(rows)
	assert sorted(rows) == ["vk_canon_table_kernel", "vk_table_mix_kernel"], p.stdout
	for kernel, (vgpr, agpr, alloc, scratch) in rows.items():
		assert scratch == 0 and agpr == 0, (kernel, vgpr, agpr, scratch)
	# as stated: the table kernel within 96 allocated registers (five waves per SIMD), the combination within 32
	assert rows["vk_canon_table_kernel"][2] <= 96, rows
	assert rows["vk_table_mix_kernel"][2] <= 32, rows
