"""CPU tier: the instantiations of vk_span_batch_kernel (vk_span_batch.hip), from the code object's resource metadata alone
-- nothing is run.  tools/kernel_regs.py compiles the unit for gfx950 and prints one line per kernel.  The kernel runs as ONE
workgroup of 512 threads per CU (its query tiles take up to all of the CU's LDS): two waves per SIMD, which 256 allocated registers
per lane allow.  A wave keeps two accumulators per staged query tile (QT = 1, 2, 4, 6, 8: up to 64 registers) and the K-blocks of two
span tiles in flight; an accumulator or a block indexed by a run-time value would move to scratch.  Skipped where hipcc is missing."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"   # the compiler tools/kernel_regs.py calls
LINE = re.compile(r"vk_span_batch_kernel<(\d+), (true|false), (\d+), (\d+)>\(.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)")
FORMS = [(10, "true", 0), (12, "false", 0), (24, "false", 0), (32, "false", 0), (0, "false", 0), (19, "false", 1), (0, "false", 1)]   # (NK, TAIL, PREC)
FILLS = (1, 2, 4, 6, 8)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: nothing to compile with")


def test_every_instantiation_fits_two_waves_per_simd_without_scratch():
	p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), os.path.join(ROOT, "vectorian_amd", "csrc", "vk_span_batch.hip")],
		cwd=ROOT, capture_output=True, text=True)
	assert p.returncode == 0, p.stderr
	rows = {(int(m[1]), m[2], int(m[3]), int(m[4])): tuple(int(x) for x in m.groups()[4:]) for m in LINE.finditer(p.stdout)}
	print(rows)
	assert sorted(rows) == sorted((nk, tail, prec, qt) for nk, tail, prec in FORMS for qt in FILLS), p.stdout
	for form, (vgpr, agpr, alloc, scratch) in rows.items():
		assert scratch == 0, (form, scratch)
		assert alloc <= 256, (form, alloc)          # two waves per SIMD: 512 registers per lane and SIMD
		# the accumulators alone: 2 span tiles x QT query tiles x 4 registers; a form far above them keeps something it should not
		assert alloc >= 8 * form[3], (form, alloc)
	# small batches stay small: a single staged query tile within 96 registers
	assert all(rows[(nk, tail, prec, 1)][2] <= 96 for nk, tail, prec in FORMS), rows
