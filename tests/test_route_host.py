"""CPU tier: the route of a single query (vectorian_amd/csrc/vk_route_host.h).  The header is host-only; a g++ driver
(AddressSanitizer, UBSan) enumerates a grid of facts -- layouts, precisions, row widths, corpus shapes, query lengths, every algorithm
form and gap family, listed slices / tracebacks / submatch weight / tag weights, every switch alone -- and holds each route against
invariants and against the validator's rule of the commit before the route existed; the named cases of route_cases.py get the routes
their kernel trace showed on that commit.  Text checks: vk_query.cpp reads no environment variable and keeps no routing boolean."""

import os
import re
import subprocess

import numpy as np
import pytest

import route_cases as rc
from test_devbuf import CSRC, ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
	exe = str(tmp_path_factory.mktemp("route_host") / "route_driver")
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
		"-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "route_driver.cpp"), "-o", exe], check=True)

	def run(what, text=""):
		return subprocess.run([exe, what], input=text, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
	return run


def test_every_route_of_the_grid_holds_its_invariants(driver):
	"""(a) one scoring plan whose kernel takes the slices of at most 64 tokens, (b) every class of slices the corpus holds claimed by
	one pass and no other, one kernel per work list, (c) refused exactly where the parent's vk_validate_query refused, (d) a switch
	takes its kernel out and leaves every route without that kernel as it was, (e) ostride 64 exactly with the wide traceback family"""
	out = driver("enumerate")
	assert not [line for line in out if line.startswith("VIOLATED")], out[:10]
	points, refused, violations = [int(x) for x in re.fullmatch(r"points (\d+) refused (\d+) violations (\d+)", out[-1]).groups()]
	assert violations == 0 and points > 2000000 and refused > 10000   # (the grid holds shapes the LDS refuses: 768-d rows in fp32)


def _ws_tail(table, max_len):
	"""vk_host::ws_tail_of, restated"""
	if max_len < 2:
		return 0
	kt = max_len
	while kt > 1 and table[kt - 1] == table[max_len]:
		kt -= 1
	return kt if kt < max_len else 0


def facts_line(name):
	"""the facts of a named case as the library would copy them from its corpus and query (the tiles two rows span: an upper bound --
	no case is near the LDS limit)"""
	corpus, d, len_t, opt, env = rc.CASES[name]
	lens = rc.lengths(corpus)
	max_len = int(lens.max())
	short = lens[lens <= 64]
	n_mid, xlong = int(((lens > 64) & (lens <= 512)).sum()), bool((lens > 512).any())
	nk32, tail = (d + 31) // 32, int(d % 32 != 0 and d % 32 <= 16)
	alg = opt.get("algorithm", rc.ALIGN)
	gap_mode, a_t, ws_tail = 0, 0.0, 0
	if alg == rc.ALIGN:
		kinds = ["table" if isinstance(g, str) else "affine" if isinstance(g, tuple) else "linear" for g in opt["gap"]]
		gap_mode = 2 if "table" in kinds else 0 if kinds == ["linear", "linear"] else 1
		a_t = float(opt["gap"][1][1]) if kinds[1] == "affine" and gap_mode == 1 else 0.0
		if gap_mode == 2:
			ws_tail = _ws_tail({"exp5": rc.exp5, "rising": rc.rising}[opt["gap"][0]](max(512, max_len))[1], max_len)
	inj, full = bool(opt.get("rwmd", (True,))[0]), bool(opt.get("wmd_full"))
	switch = {"VK_LONG_PASS": 1, "VK_NO_APART": 10, "VK_NO_SCORE32": 11}[next(iter(env))] if env else -1
	v = [1 if corpus == "E" else 0, 0, nk32, tail, max_len, int(short.max()), n_mid, int(n_mid > 0 or xlong), int(xlong), 2 * ((max_len + 15) // 16) + 1,
		2 * ((int(short.max()) + 15) // 16) + 1, 1 if corpus == "D" else 0, 0, alg, int(full), int(inj and alg == rc.RWMD), len_t, gap_mode, a_t, ws_tail,
		int("submatch_weight" in opt), int(bool(opt.get("tagged"))), int("only" in opt), 1, opt.get("locality", 0), 14, 1, 0, switch]
	return " ".join(str(x) for x in v)


def test_named_cases_take_the_routes_of_the_parents_kernel_trace(driver):
	names = sorted(rc.CASES)
	assert len(names) >= 30 and set(names) == set(rc.ROUTES)
	out = driver("route", "\n".join(facts_line(n) for n in names) + "\n")
	assert len(out) == len(names)
	for name, line in zip(names, out):
		t = line.split()
		assert t[14:16] == ["status", "0"], (name, line)
		rc.check_route(name, dict(zip(rc.STATE, [int(x) for x in t[:14]])))


def test_exp5_saturates_where_the_cases_say():
	assert _ws_tail(rc.exp5(512)[1], 200) == 125 and _ws_tail(rc.exp5(512)[1], 64) == 0 and _ws_tail(rc.rising(600)[1], 600) == 0
	assert _ws_tail(np.zeros(100, np.float32), 64) == 1   # a constant cost: its tail begins at once


def test_the_query_unit_decides_no_route_of_its_own():
	text = open(os.path.join(CSRC, "vk_query.cpp")).read()
	assert "getenv" not in text   # the switches are read in one place: vk_host::read_route_switches
	assert open(os.path.join(CSRC, "vk_route_host.h")).read().count("getenv(") == 1
	for gone in ("long_via_wide", "wide_score", "rwmd_long_doc", "doc_fast", "flow_doc", "docg_ok", "doc_ok", "rwmd_inj", "long_apart", "docw_rwmd",
			"apart_route", "two_blocks", "wide_sub", "score32_plan", "Score32Plan", "transport_in_lds"):
		assert not re.search(r"\b%s\b" % gone, text), gone
	# the query's path: the context, its stages and query_body
	body = text[text.index("struct query_run {"):text.index('extern "C" {')]
	assert "static int query_body(" in body
	assert body.count("vk_host::route_query(") == 1 and body.index("vk_host::route_query(") < body.index("hipEventRecord(c->ev[0]")
	assert not re.search(r"\bwp\.gap_mode = [^r]", body) and "does not fit this corpus (LDS)" not in text
	# wp is built once: every assignment to one of its fields sits in build_wide(), and the one launch under another gap mode -- the
	# multi-block kernel's -- sets it on a copy (no stage hands wp itself to a launch: each works on a copy of its own)
	built = body[body.index("void build_wide() {"):body.index("int prepare() {")]
	assert len(re.findall(r"\bwp\.\w+ = |memcpy\(wp\.", built)) == len(re.findall(r"\bwp\.\w+ = |memcpy\(wp\.", body)) > 0
	assert "&wp" not in body and re.findall(r"(\w+)\.gap_mode = r\.score32_gap_mode", body) == ["mb"]
	multi = body[body.index("int score_multi_block() {"):body.index("int score_span() {")]
	assert "VkWideParams mb = wp;" in multi and re.findall(r"(\w+)\.gap_mode = r\.(?:wide|score32)_gap_mode", body) == ["wp", "mb"]


def test_the_names_are_the_headers():
	"""route_cases.py names the enums of vk_route_host.h and the order of vk_query_route_index: read from the two headers"""
	route = open(os.path.join(CSRC, "vk_route_host.h")).read()
	for enum, prefix, names in (("route_plan", "PLAN_", rc.PLAN), ("route_pass", "PASS_", rc.PASS), ("route_list", "LIST_", rc.LIST), ("route_flow", "FLOW_", rc.FLOW)):
		body = re.search(r"enum %s \{([^}]*)\}" % enum, route).group(1)
		assert [x.strip() for x in body.split(",")] == [prefix + n for n in names]
	body = re.search(r"enum vk_query_route_index \{([^}]*)\}", open(os.path.join(CSRC, "vk_internal.h")).read()).group(1)
	assert [x.strip() for x in body.split(",") if x.strip()] == ["VK_QR_" + n.upper() for n in rc.STATE] + ["VK_QR_COUNT"]
