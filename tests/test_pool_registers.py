"""CPU tier: the instantiations of vk_pool_spans_kernel (vk_pool.hip), from the code object's resource metadata alone --
nothing is run.  tools/kernel_regs.py compiles the unit for gfx950 and prints one line per kernel.  A wave keeps the accumulators of
four feature chunks and four rows of each in flight; an accumulator or a row indexed by a run-time value would move to scratch.  The
kernel is bound by the bytes of the rows, and what hides their latency is the rows in flight per wave times the waves per SIMD: the
16-byte forms stay within 128 registers (four waves per SIMD), the element forms within 64.  Skipped where hipcc is missing."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"   # the compiler tools/kernel_regs.py calls
LINE = re.compile(r"vk_pool_spans_kernel<(\d+), (true|false), (unsigned short|float), (\d+)>\(.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: nothing to compile with")


def test_every_instantiation_runs_without_scratch():
	p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), os.path.join(ROOT, "vectorian_amd", "csrc", "vk_pool.hip")],
		cwd=ROOT, capture_output=True, text=True)
	assert p.returncode == 0, p.stderr
	rows = {(int(m[1]), m[2], m[3], int(m[4])): tuple(int(x) for x in m.groups()[4:]) for m in LINE.finditer(p.stdout)}
	print(rows)
	# AGG x GATHER x the rows' type x features per lane and load
	assert sorted(rows) == sorted((agg, gather, t, vec) for agg in (0, 1, 2) for gather in ("true", "false") for t in ("float", "unsigned short") for vec in (1, 4)), p.stdout
	for form, (vgpr, agpr, alloc, scratch) in rows.items():
		assert scratch == 0, (form, scratch)
		assert agpr == 0, (form, agpr)
		assert alloc <= (128 if form[3] == 4 else 64), (form, alloc)
		# four rows of four chunks in flight beside the accumulators: a form far below them has lost its loads in flight
		assert alloc >= 5 * 4 * form[3], (form, alloc)
