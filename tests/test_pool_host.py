"""CPU tier: the pooled span vectors of vectorian_amd/csrc/vk_pool_host.h against numpy.  A g++ driver with its own main
(tests/pool_driver.cpp), built plain and with AddressSanitizer / UBSan and run as a stand-alone program, computes the header's cell for
every width and span length of pool_cases.py: the MEAN bit for bit what np.mean(v, axis=0) returns on the span's float32 rows, MIN and
MAX value-equal to np.min / np.max with NaN in the same places.  The same inputs show that another order of the sum could not pass:
summed backwards, pairwise or in float64, a quarter or more of a row's cells differ.  The geometry of vk_pool_spans_kernel's grid is
walked on the host: every span and every feature exactly once."""

import os
import re
import subprocess

import numpy as np
import pytest

import pool_cases as pc
from test_devbuf import CSRC, ROOT

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
	work = tmp_path_factory.mktemp("pool_" + request.param)
	exe = str(work / "pool_driver")
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (SANITIZE if request.param == "sanitized" else []) +
		["-I", CSRC, os.path.join(ROOT, "tests", "pool_driver.cpp"), "-o", exe], check=True)

	def run(*args):
		return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
	run.work = work
	return run


def pooled_by_the_header(driver, rows, ids, start, end):
	"""{agg name: [n_spans x d]} from the driver"""
	d, n_spans = rows.shape[1], len(start)
	src, dst = str(driver.work / "in.bin"), str(driver.work / "out.bin")
	with open(src, "wb") as f:
		for a in (rows, np.zeros(0, np.int32) if ids is None else ids.astype(np.int32), start.astype(np.int64), end.astype(np.int64)):
			f.write(np.ascontiguousarray(a).tobytes())
	r = driver("pool", int(rows.dtype == np.uint16), d, rows.shape[0], 0 if ids is None else len(ids), n_spans, src, dst)
	assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-3000:])
	out = np.fromfile(dst, dtype=np.float32).reshape(3, n_spans, d)
	return dict(zip(("mean", "min", "max"), out))


@pytest.mark.parametrize("d", pc.WIDTHS)
def test_the_cell_is_numpys(driver, d):
	"""rows as they are and gathered through ids (repeated ids, a zero row), fp32; spans of every length, overlapping, one empty in the
	middle, one NaN component"""
	for case in (pc.rows_case(d), pc.gather_case(d)):
		got = pooled_by_the_header(driver, case["rows"], case["ids"], case["start"], case["end"])
		for agg, want in pc.expected(case).items():
			pc.assert_pooled(got[agg], want, agg, (d, case["name"]))


@pytest.mark.parametrize("d", [4, 17, 300])
def test_bf16_rows_are_widened_exactly(driver, d):
	case = pc.rows_case(d, bf16=True)
	got = pooled_by_the_header(driver, case["rows"], None, case["start"], case["end"])
	for agg, want in pc.expected(case).items():
		pc.assert_pooled(got[agg], want, agg, d)


def test_another_order_of_the_sum_cannot_pass():
	"""the inputs tell the orders apart: for every span of at least 8 tokens at d >= 64 the mean summed backwards, pairwise (a tree) or
	in float64 and rounded once differs from np.mean's in at least a quarter of the row's cells.  Inputs that do not are rejected."""
	checked = 0
	for d in (d for d in pc.WIDTHS if d >= 64):
		case = pc.rows_case(d)
		rows, want = case["rows"], pc.expected(case)["mean"]
		for i, (a, b) in enumerate(zip(case["start"], case["end"])):
			if b - a < 8:
				continue
			v = rows[a:b]
			others = dict(backwards=pc.sequential_mean(v[::-1]), pairwise=pc.pairwise_mean(v), float64=v.astype(np.float64).mean(axis=0).astype(np.float32))
			for name, other in others.items():
				differing = float((other.view(np.uint32) != want[i].view(np.uint32)).mean())
				assert differing >= 0.25, (d, i, int(b - a), name, differing)
			checked += 1
	assert checked == 8 * len([d for d in pc.WIDTHS if d >= 64])


def test_numpy_sums_a_span_row_by_row():
	"""what the header states about np.mean holds for the numpy of this machine: a sequential fp32 sum in token order, divided once"""
	for d in (2, 3, 64, 300):
		case = pc.rows_case(d)
		want = pc.expected(case)["mean"]
		for i, (a, b) in enumerate(zip(case["start"], case["end"])):
			if b > a:
				assert np.array_equal(pc.sequential_mean(case["rows"][a:b]).view(np.uint32), want[i].view(np.uint32)), (d, i)


def test_every_span_and_feature_is_covered_once(driver):
	r = driver("geometry")
	out = r.stdout.split("\n")[:-1]
	assert r.returncode == 0 and not [line for line in out if line.startswith("VIOLATED")], (out[:10], r.stderr[-2000:])
	points, violations = [int(x) for x in re.fullmatch(r"points (\d+) violations (\d+)", out[-1]).groups()]
	assert violations == 0 and points == (23 + 10) * 12


def test_spans_and_ids_are_checked_before_anything_runs(driver):
	"""pool_check_spans, the validation of vk_corpus_append_pooled: 0 ok, 1 invalid, 2 unsupported"""
	def check(n_rows, ids, start, end):
		src = str(driver.work / "check.bin")
		with open(src, "wb") as f:
			for a, t in ((ids if ids is not None else [], np.int32), (start, np.int64), (end, np.int64)):
				f.write(np.asarray(a, dtype=t).tobytes())
		r = driver("check", n_rows, 0 if ids is None else len(ids), len(start), src)
		assert r.returncode == 0, r.stderr[-2000:]
		return int(r.stdout.split()[0])
	assert check(10, None, [0, 3, 3, 2], [3, 3, 10, 9]) == 0
	assert check(10, None, [4], [3]) == 1            # start > end
	assert check(10, None, [0], [11]) == 1           # outside the rows
	assert check(10, None, [-1], [2]) == 1
	assert check(3, [0, 2, 2, 1], [0, 1], [4, 4]) == 0
	assert check(3, [0, 2, 2, 1], [0], [5]) == 1     # outside the ids
	assert check(3, [0, 3, 2, 1], [0], [4]) == 1     # an id outside the rows
	assert check(3, [0, -1, 2, 1], [0], [4]) == 1
	assert check((1 << 24) + 1, None, [0], [1 << 24]) == 0
	assert check((1 << 24) + 1, None, [0], [(1 << 24) + 1]) == 2   # (float)n is not exact


def test_the_kernel_and_the_entry_point_read_the_header():
	kernel, corpus = [open(os.path.join(CSRC, name)).read() for name in ("vk_pool.hip", "vk_corpus.cpp")]
	assert '#include "vk_pool_host.h"' in kernel and '#include "vk_pool_host.h"' in corpus
	for name in ("pool_fold<", "pool_finish<", "pool_span_of(", "pool_feature_of(", "pool_passes(", "pool_grid(", "pool_vec("):
		assert "vk_host::" + name in kernel, name
	assert "vk_host::pool_check_spans(" in corpus
	assert "#define VK_ABI_VERSION 12" in open(os.path.join(ROOT, "include", "vectorian_hip.h")).read()
