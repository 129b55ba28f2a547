"""CPU tier: the registers of the scoring kernels of a contextual handle under an operator chain, from the compiler's
resource remarks alone -- nothing is run.  tools/kernel_regs.py compiles the three units of the fused forms (vk_score_m10 / m11 / m12:
MODE 10 / 11 / 12 of vk_score_kernel, every gap form and padded query length) and vk_score32.hip for gfx950.  The fused forms use no
scratch and allocate at most 168 registers: three waves per SIMD, which launch_sized's stream cap asks for.  Every chain form of
vk_score32_kernel is present beside its parent, stays in its parent's occupancy class (amdgpu_waves_per_eu as declared: two waves per
SIMD, three for the twelve-wave form) and has no scratch where the parent has none.  Skipped where hipcc is missing."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"   # the compiler tools/kernel_regs.py calls
FUSED = re.compile(r"vk_score_kernel<(\d+), 0, false, (\d+), (\d+)>.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)")
MULTI = re.compile(r"vk_score32_kernel<(\d+), (true|false), (\d+), (true|false), (\d+), (true|false)>.*vgpr\s+(\d+)\s+agpr\s+(\d+)\s+alloc\s+(\d+).*scratch\s+(\d+)\s+occ\s+(\d+)")
GAPS, LTS = (0, 1, 2, 3, 4, 5, 6, 7), (4, 8, 12, 16)
# (GAP, NB, B3, NWMAX) of the contextual forms vk_launch_score32 selects
MULTI_FORMS = [(g, nb, False, 4) for g in (0, 1, 4, 7, 5) for nb in (4, 2)] + [(g, nb, b3, 4) for g in (3, 6) for nb in (4, 2) for b3 in (True, False)] + [(3, 4, True, 12)]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc: nothing to compile with")


@pytest.fixture(scope="module")
def reports():
	units = {"vk_score_m10.hip": [], "vk_score_m11.hip": [], "vk_score_m12.hip": [],
		"vk_score32.hip": ["--", "-mllvm", "-pragma-unroll-threshold=131072"]}   # (the unit's own flag: vectorian_amd/csrc/Makefile)
	procs = {u: subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), os.path.join(ROOT, "vectorian_amd", "csrc", u)] + extra,
		cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for u, extra in units.items()}
	out = {}
	for u, p in procs.items():
		text, err = p.communicate()
		assert p.returncode == 0, err
		print(text)
		out[u] = text
	return out


@pytest.mark.parametrize("mode", [10, 11, 12])
def test_fused_chain_forms_fit_three_waves_per_simd_without_scratch(reports, mode):
	rows = {tuple(int(x) for x in m.groups()[:3]): tuple(int(x) for x in m.groups()[3:]) for m in FUSED.finditer(reports["vk_score_m%d.hip" % mode])}
	assert sorted(rows) == [(mode, gap, lt) for gap in GAPS for lt in LTS], sorted(rows)
	for (_, gap, lt), (vgpr, agpr, alloc, scratch) in sorted(rows.items()):
		assert alloc == (vgpr + agpr + 7) // 8 * 8
		assert scratch == 0, (mode, gap, lt, scratch)
		assert alloc <= 168, (mode, gap, lt, vgpr, agpr, alloc)


def test_multi_block_chain_forms_stay_in_their_parents_class(reports, record_property):
	rows = {}
	for m in MULTI.finditer(reports["vk_score32.hip"]):
		g = m.groups()
		rows[(int(g[0]), g[1] == "true", int(g[2]), g[3] == "true", int(g[4]), g[5] == "true")] = tuple(int(x) for x in g[6:])
	chain = sorted(k for k in rows if k[5])
	assert chain == sorted((g, False, nb, b3, nw, True) for g, nb, b3, nw in MULTI_FORMS), chain   # contextual forms only, every one of them
	for key in chain:
		parent = key[:5] + (False,)
		assert parent in rows, parent
		vgpr, agpr, alloc, scratch, occ = rows[key]
		_, _, p_alloc, p_scratch, p_occ = rows[parent]
		declared = 3 if key[4] > 4 else 2
		record_property("vk_score32_kernel<%d, %s, %d, %s, %d, %s>" % key, "alloc %d (parent %d) scratch %d (parent %d) waves/SIMD %d (parent %d)" % (alloc, p_alloc, scratch, p_scratch, occ, p_occ))
		# the class is the declared one: a parent that happens to fit a third wave (165 registers, <3, false, 4, true, 4>) declares two
		assert occ >= declared and p_occ >= declared, (key, occ, p_occ)
		assert alloc <= 512 // declared, (key, alloc)
		assert p_scratch > 0 or scratch == 0, (key, scratch, p_scratch)
