"""CPU tier: the host side of the span similarity (vectorian_amd/csrc/vk_span_sim_host.h).  A g++ driver with its own main
(tests/span_sim_driver.cpp), built plain and with AddressSanitizer / UBSan and run as a stand-alone program:
  * the cell of a source AS THE KERNEL STREAMS IT -- both sides zero-padded to whole blocks of 16 features, one double partial sum
    per lane, the two exchanges -- equals vk_host::sim_src_cell bit for bit, in all four forms (p = 1, p = 2, general p, the
    sqrt-cosine), at every width where the padding or the number of blocks changes, for rows of three magnitudes, a zero row, a row
    equal to the query and its negative, a zero query; a row of NaN gives NaN under a p-norm.  That the padding's +0.0 terms leave
    a sum's bits is therefore measured, not assumed;
  * the grid walk visits every tile exactly once, 1 .. 2^20 spans, a sweep of the grid more or less among them;
  * the floor of the selection and the predicate "this query is span-shaped", case by case."""

import os
import re
import subprocess

import pytest

from test_devbuf import CSRC, ROOT

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
WIDTHS = 19    # d in {1..5, 7, 8, 15, 16, 17, 31, 32, 33, 64, 67, 100, 300, 768, 1024}
SOURCES = 5    # p = 1, 2, 3, 0.5 and the sqrt-cosine: the four forms, the general one twice
ROWS = 27      # 24 random rows, a zero row, the query, its negative


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
	exe = str(tmp_path_factory.mktemp("span_sim_" + request.param) / "span_sim_driver")
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + (SANITIZE if request.param == "sanitized" else []) +
		["-I", CSRC, os.path.join(ROOT, "tests", "span_sim_driver.cpp"), "-o", exe], check=True)
	return lambda *args: subprocess.run([exe, *args], capture_output=True, text=True)


def test_the_streamed_cell_is_the_headers_cell(driver):
	r = driver()
	out = r.stdout.split("\n")[:-1]
	assert r.returncode == 0, (out[:10], r.stderr[-2000:])
	cells, mismatches, nan_ok = [int(x) for x in re.fullmatch(r"cells (\d+) mismatches (\d+) nan_ok (\d+)", out[-1]).groups()]
	assert mismatches == 0 and cells == WIDTHS * SOURCES * ROWS * 2 and nan_ok == WIDTHS * SOURCES, out[:10]


def test_the_grid_walk_visits_every_tile_once(driver):
	r = driver("walk")
	out = r.stdout.split("\n")[:-1]
	assert r.returncode == 0, (out[:10], r.stderr[-2000:])
	walks, violations = [int(x) for x in re.fullmatch(r"walks (\d+) violations (\d+)", out[-1]).groups()]
	assert violations == 0 and walks > 6 * 2100


def test_the_grid(driver):
	grid = lambda n, cus: int(driver("grid", str(n), str(cus)).stdout)
	# one wave per run of four tiles, four waves per workgroup: 256 spans per workgroup; at most three workgroups per CU
	assert [grid(n, 256) for n in (1, 256, 257, 3001, 256 * 768, 256 * 768 + 1, 1 << 20)] == [1, 1, 2, 12, 768, 768, 768]
	assert [grid(n, 1) for n in (1, 256, 257, 513, 769, 1 << 20)] == [1, 1, 2, 3, 3, 3]


def test_the_staged_query_and_the_raw_tile(driver):
	sizes = lambda d: tuple(int(x) for x in driver("lds", str(d)).stdout.split())
	assert [sizes(d) for d in (1, 16, 17, 300, 768, 1024)] == [(64, 1024), (64, 1024), (128, 2048), (19 * 64, 19 * 1024), (48 * 64, 48 * 1024), (4096, 65536)]


@pytest.mark.parametrize("min_score,floor", [(0.0, 0.0), (0.25, 0.25), (-1.0, 0.0), (-0.0, 0.0), (float("nan"), 0.0), (float("-inf"), 0.0), (3.5, 3.5)])
def test_the_floor(driver, min_score, floor):
	assert float.fromhex(driver("floor", repr(min_score)).stdout.strip()) == floor


ALIGN, RWMD, WRD = 0, 1, 2
LOCAL, GLOBAL, SEMIGLOBAL = 0, 1, 2
SHAPED = dict(algorithm=ALIGN, locality=LOCAL, len_t=1, uniform_len=1, tagged=0, submatch=0, boost=0, want_flow=0, only=0, sim_rows=0)


@pytest.mark.parametrize("change,words", [
	({}, "ok"),
	(dict(len_t=2), "more than one token"),
	(dict(uniform_len=0), "one row"),
	(dict(uniform_len=3), "one row"),
	(dict(algorithm=RWMD), "VK_ALG_RWMD"),
	(dict(algorithm=WRD), "VK_ALG_ALIGN"),
	(dict(locality=GLOBAL), "global alignment"),
	(dict(locality=SEMIGLOBAL), "not local"),
	(dict(tagged=1), "tag weights"),
	(dict(submatch=1), "submatch weight"),
	(dict(boost=1), "booster"),
	(dict(want_flow=1), "want_flow"),
	(dict(only=1), "only_slices"),
	(dict(sim_rows=1), "similarity rows"),
])
def test_which_queries_are_span_shaped(driver, change, words):
	q = dict(SHAPED, **change)
	r = driver("shape", *[str(q[k]) for k in ("algorithm", "locality", "len_t", "uniform_len", "tagged", "submatch", "boost", "want_flow", "only", "sim_rows")])
	assert r.returncode == 0 and words in r.stdout, r.stdout


def test_the_route_and_the_kernels_read_the_header():
	"""one place computes these numbers"""
	query, kernel, internal, corpus = [open(os.path.join(CSRC, name)).read() for name in ("vk_query.cpp", "vk_span_sim.hip", "vk_internal.h", "vk_corpus.cpp")]
	assert '#include "vk_span_sim_host.h"' in kernel and '#include "vk_span_sim_host.h"' in internal
	for name in ("span_sim_refusal(", "span_sim_floor("):
		assert "vk_host::" + name in query, name
	for name in ("span_sim_grid(", "span_sim_first_run(", "span_sim_run_stride(", "span_sim_run_end(", "span_sim_lds_bytes(", "kSpanSimDepth"):
		assert "vk_host::" + name in kernel, name
	assert "vk_host::span_sim_raw_tile_bytes(" in corpus
