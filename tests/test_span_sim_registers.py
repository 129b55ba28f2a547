"""CPU tier: the instantiations of vk_span_sim_kernel and vk_span_ops_kernel (vk_span_sim.hip), from the code object's
resource metadata alone -- nothing is run.  tools/kernel_regs.py compiles the unit for gfx950 and prints one line per kernel.  Both
kernels are bound by the bytes of the rows and are launched three workgroups of four waves per CU, as vk_span_kernel is: three waves
per SIMD need at most 168 VGPRs (accumulation registers included), and a block of loads indexed by a run-time value would move to
scratch.  Skipped where hipcc is missing."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"   # the compiler tools/kernel_regs.py calls
LINE = re.compile(r"(vk_span_sim_kernel<(\d+)>|vk_span_ops_kernel)\(.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: nothing to compile with")


def test_every_instantiation_runs_three_waves_per_simd_without_scratch():
	p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), os.path.join(ROOT, "vectorian_amd", "csrc", "vk_span_sim.hip")],
		cwd=ROOT, capture_output=True, text=True)
	assert p.returncode == 0, p.stderr
	rows = {("ops" if m[2] is None else int(m[2])): tuple(int(x) for x in m.groups()[2:]) for m in LINE.finditer(p.stdout)}
	print(rows)
	# p = 1, p = 2, general p, the sqrt-cosine (vk_host::SIM_SRC_*), and the cosine under a chain
	assert sorted(rows, key=str) == [0, 1, 2, 3, "ops"], p.stdout
	for form, (vgpr, agpr, alloc, scratch) in rows.items():
		assert scratch == 0, (form, scratch)
		assert alloc <= 168, (form, alloc)
		# eight blocks of 16 bytes per lane in flight before the first use (the sources), four K-steps and the query's (the cosine)
		assert alloc >= 32, (form, alloc)
