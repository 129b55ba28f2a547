"""CPU tier: the geometry of vk_longq_kernel (vectorian_amd/csrc/vk_longq_host.h).  The header is host-only; a g++ driver
(AddressSanitizer, UBSan) enumerates every query length 65 .. 512, longest slice 1 .. 512, gap mode, tracebacks or not, tag weights or
not: the LDS of a launch stays within 160 KB and its parts (canon staging, strip, border columns, matrix) do not overlap; the parts of
a scratch region (matrix, records, similarities) do not overlap and lie inside it; grids are at least 1; and for a longest slice of at
most 64 tokens every value is what vk_longq_stride / vk_longq_scratch_bytes / vk_longq_lds_bytes / vk_longq_blocks returned before the
header existed.  The border columns of the block form are in LDS for every shape: the largest launch is printed and held here."""

import os
import re
import subprocess

import pytest

from test_devbuf import CSRC, ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
	exe = str(tmp_path_factory.mktemp("longq_geometry") / "longq_geometry_driver")
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
		"-I", CSRC, os.path.join(ROOT, "tests", "longq_geometry_driver.cpp"), "-o", exe], check=True)
	return lambda *args: subprocess.run([exe, *args], capture_output=True, text=True)


def test_every_shape_holds_its_invariants(driver):
	r = driver()
	out = r.stdout.split("\n")[:-1]
	assert r.returncode == 0 and not [line for line in out if line.startswith("VIOLATED")], (out[:10], r.stderr[-2000:])
	points, violations = [int(x) for x in re.fullmatch(r"points (\d+) violations (\d+)", out[-1]).groups()]
	assert violations == 0 and points == 448 * 512 * 3 * 2 * 2


def test_the_largest_launch_and_region(driver):
	"""512 query tokens over a 512-token slice: strip 128 KB + canon 8 KB + two border columns of H and E (8,208 bytes) + 64 -- the columns
	fit the LDS beside the strip of a traceback launch, so no shape puts them in the scratch region; a region is 2.6 MB"""
	lds, scratch = [int(x) for x in re.fullmatch(r"lds (\d+) scratch (\d+)\n", driver("worst").stdout).groups()]
	assert lds == 512 * 64 * 4 + 8192 + 2 * 2 * 513 * 4 + 64 <= 160 * 1024
	assert scratch == (513 * 512 * 4 + 513 * 512 * 2 + 512 * 512 * 4 + 255) // 256 * 256 + 256


def test_the_kernel_units_and_the_host_read_the_header():
	"""one place computes these numbers: the kernel units keep no geometry of their own, the host unit sizes its buffers from the header"""
	short, blocks, shared, host = [open(os.path.join(CSRC, name)).read() for name in ("vk_longq.hip", "vk_longq_blocks.hip", "vk_longq.hip.h", "vk_longq_host.cpp")]
	assert '#include "vk_longq_host.h"' in shared and '#include "vk_longq_host.h"' in host
	assert '#include "vk_longq.hip.h"' in short and '#include "vk_longq.hip.h"' in blocks
	assert "struct VkLongqGeom" not in short and "160 * 1024" not in short + blocks
	for text in (short, blocks, host):
		assert "vk_host::longq_geometry_of(" in text
	assert "static_assert(vk_host::kLongqCanonLds == VK_CANON_LDS" in shared
