"""CPU tier: from the selected keys and their tracebacks to a result set (vectorian_amd/csrc/vk_result_host.h) -- the key codec, the
order of a result set, the score of a winner restated from its traceback, the forms of the gap costs.  The header is host-only; a g++
driver (AddressSanitizer, UBSan) runs each rule on inputs from this file, and the answers are held, as bit patterns, against the rule
stated here in numpy float32.  Text checks: the three query units carry no copy of these rules of their own."""

import ctypes
import ctypes.util
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import vk_oracle as vo
from test_devbuf import CSRC, HOST_UNITS, ROOT, _enclosing_functions

F = np.float32
QUERY_UNITS = ("vk_query.cpp", "vk_batch.cpp", "vk_longq_host.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
	exe = str(tmp_path_factory.mktemp("result_host") / "result_host_driver")
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
		"-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "result_host_driver.cpp"), "-o", exe], check=True)

	def run(what, *numbers):
		out = subprocess.run([exe, what], input=" ".join(str(x) for x in numbers), check=True, capture_output=True, text=True)
		return out.stdout.split("\n")[:-1]
	return run


def hexbits(x):
	return "%08x" % int(np.asarray(x, dtype=F).view(np.uint32))


def encode(score, row):
	"""a selection key as the kernels make it: float_orderable (vk_select.hip:17) of the score above the row"""
	u = int(np.asarray(score, dtype=F).view(np.uint32))
	ob = (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)
	return (ob << 32) | row


def test_key_codec_inverts_the_encoder_bit_for_bit(driver):
	tiny = np.uint32(1).view(F)   # the smallest denormal
	scores = [F(1.5), F(-1.5), F(0.0), F(-0.0), tiny, -tiny, np.uint32(0x007fffff).view(F), F(np.inf), F(-np.inf), F(3.4e38), F(-3.4e38), F(1e-30), F(0.3)]
	rows = [0, 1, 7, 0xffffffff, 12345, 2 ** 31, 2 ** 31 - 1, 3, 4, 5, 6, 8, 9]
	keys = [encode(s, r) for s, r in zip(scores, rows)]
	out = driver("codec", len(keys), *keys)
	for line, s, r in zip(out, scores, rows):
		assert line == "%s %d" % (hexbits(s), r)
	assert out[len(keys)] == "count %d" % len(keys)   # no encoded score gives the empty slot's 0
	assert [int(x) for x in out[len(keys) + 1:]] == [(1 << 32) | r for r in rows]   # the key that names a listed row
	assert driver("codec", 5, keys[0], keys[1], 0, keys[2], 0)[5] == "count 2"   # up to the FIRST empty slot
	assert driver("codec", 1, 0)[1] == "count 0"


def test_key_order_is_score_then_row(driver):
	"""keys compared as unsigned 64-bit numbers, descending, come in the order of a result set (-0.0 left out: as a key it sorts below
	+0.0, as a score it ties with it)"""
	rng = np.random.default_rng(5)
	scores = np.concatenate([rng.standard_normal(40).astype(F), [F(0.0), F(np.inf), F(1e-40), F(-1e-40), F(-3e38)]]).astype(F)
	scores = np.concatenate([scores, scores[:20]])   # exact ties
	rows = rng.permutation(len(scores)).astype(np.int64) * 1000003 % (2 ** 32)
	keys = [encode(s, int(r)) for s, r in zip(scores, rows)]
	by_key = sorted(range(len(keys)), key=lambda i: keys[i], reverse=True)
	out = driver("rank", hexbits(-np.inf), len(keys), *[x for s, r in zip(scores, rows) for x in (hexbits(s), int(r))])
	assert [int(x) for x in out] == by_key


def test_rank_is_the_documented_total_order(driver):
	"""above min_score only (a score EQUAL to it is out); score descending; ties by slice index descending"""
	min_score = F(0.25)
	scores = [F(0.5), F(0.25), F(0.75), F(0.5), F(0.1), F(0.5), F(np.inf), F(0.25000003), F(-1.0), F(0.75), F(0.0), F(-0.0)]
	slices = [10, 11, 3, 2 ** 40, 5, 7, 0, 1, 2, 2 ** 33 + 3, 8, 9]   # (the merges rank 64-bit slice indices)
	kept = [i for i in range(len(scores)) if scores[i] > min_score]
	want = sorted(kept, key=lambda i: (-float(scores[i]), -slices[i]))
	assert want == [6, 9, 2, 3, 0, 5, 7]
	out = driver("rank", hexbits(min_score), len(scores), *[x for s, r in zip(scores, slices) for x in (hexbits(s), r)])
	assert [int(x) for x in out] == want
	# below zero the two zeros tie and the slice decides
	out = driver("rank", hexbits(-0.5), 2, hexbits(-0.0), 4, hexbits(0.0), 3)
	assert [int(x) for x in out] == [0, 1]


def _powf(x, y):
	libm = ctypes.CDLL(ctypes.util.find_library("m"))
	libm.powf.restype = ctypes.c_float
	libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
	return F(libm.powf(float(x), float(y)))


def _reference_score(raw, mapping, tag_weights, total, w, boost):
	"""vko_score (oracle/vk_oracle.c), each operation rounded to float32, with the matched weight summed over the query in order"""
	matched = F(0.0)
	for j, m in enumerate(mapping):
		if m >= 0:
			matched = F(matched + (tag_weights[j] if tag_weights is not None else F(1.0)))
	unmatched = _powf(F(F(total - matched) / total), w)
	ref = F(matched + F(unmatched * F(total - matched)))
	return F(F(raw / ref) * boost)


def test_reference_score_is_the_oracles_float_for_float(driver):
	rng = np.random.default_rng(11)
	numbers, want, unit = [], [], []
	for case in range(400):
		len_t = int(rng.integers(1, 65))
		tagged = case % 2 == 1
		w = F(0.0) if case % 4 < 2 else F(0.5)
		mapping = np.where(rng.random(len_t) < rng.random(), rng.integers(0, 500, len_t), -1).astype(np.int16)
		if case % 16 == 0:
			mapping[:] = 3    # every token matched: base 0 of the power
		if case % 16 == 2:
			mapping[:] = -1   # nothing matched: base 1
		tw = rng.uniform(0.1, 2.0, len_t).astype(F)
		total = F(len_t)
		if tagged:
			total = F(0.0)
			for t in tw:
				total = F(total + t)
		raw = F(rng.uniform(0.0, len_t))
		boost = F(1.0) if case % 3 else F(rng.uniform(0.5, 2.0))
		numbers += [hexbits(raw), hexbits(total), hexbits(w), hexbits(boost), len_t, int(tagged), *[int(m) for m in mapping], *[hexbits(t) for t in tw]]
		want.append(hexbits(_reference_score(raw, mapping, tw if tagged else None, total, w, boost)))
		unit.append(None if tagged else hexbits(vo.score(float(raw), len_t, int((mapping >= 0).sum()), float(w), float(boost))))
	got = driver("score", 400, *numbers)
	assert got == want
	# ... and, with unit weights, the oracle's own vko_score
	assert [g for g, u in zip(got, unit) if u is not None] == [u for u in unit if u is not None]


def test_no_flow_fills_one_winner_and_nothing_else(driver):
	out = driver("no_flow", 5)
	assert out == ["7 %s" % hexbits(7.0)] + ["-1 %s" % hexbits(0.0)] * 5 + ["7 %s" % hexbits(7.0)]


def test_gap_classification_of_the_nine_kind_pairs(driver):
	LINEAR, AFFINE, TABLE = 0, 1, 2
	u_s, v_s, u_t, v_t = F(0.3), F(0.07), F(0.2), F(0.11)
	pairs = [(ks, kt) for ks in (LINEAR, AFFINE, TABLE) for kt in (LINEAR, AFFINE, TABLE)]
	out = driver("gaps", len(pairs), *[x for ks, kt in pairs for x in (ks, hexbits(u_s), hexbits(v_s), kt, hexbits(u_t), hexbits(v_t))])
	zero = F(0.0)
	for line, (ks, kt) in zip(out, pairs):
		if TABLE in (ks, kt):      # the kernels read the tables
			mode, fields = 2, [zero] * 6
		elif ks == LINEAR and kt == LINEAR:   # w(k) = u k
			mode, fields = 0, [u_s, u_t, zero, zero, zero, zero]
		else:                      # w(k) = u + v k; a linear side opens at 0 and extends by u
			a_s, g_s = (u_s, v_s) if ks == AFFINE else (zero, u_s)
			a_t, g_t = (u_t, v_t) if kt == AFFINE else (zero, u_t)
			mode, fields = 1, [g_s, g_t, a_s, a_t, F(a_s + g_s), F(a_t + g_t)]
		assert line == " ".join([str(mode)] + [hexbits(x) for x in fields]), (ks, kt)


def _closure(driver, table, len_t, is_align=1):
	out = driver("closure", len_t, is_align, len(table), *[hexbits(x) for x in table])
	wt = np.array([int(x, 16) for x in out], dtype=np.uint32).view(F)
	assert len(wt) == 160
	return wt[:80], wt[80:]


def test_closure_of_w_t(driver):
	len_t = 64
	k = np.arange(0, 80, dtype=F)
	# a linear cost handed over as a table is its own closure (steps of 2^-2: every sum is exact in float32)
	linear = (F(0.25) * k).astype(F)
	given, closed = _closure(driver, linear, len_t)
	want = np.where(np.arange(80) <= len_t, linear, F(0.0)).astype(F)   # as given up to the query's length, 0 beyond
	assert (given.view(np.uint32) == want.view(np.uint32)).all()
	assert (closed.view(np.uint32) == want.view(np.uint32)).all()
	# a convex cost: the closure is subadditive, never above the table, and what the table's own splits give
	convex = (F(0.01) * k * k).astype(F)
	given, closed = _closure(driver, convex, len_t)
	assert (given[:len_t + 1].view(np.uint32) == convex[:len_t + 1].view(np.uint32)).all()
	for n in range(2, len_t + 1):
		for a in range(1, n):
			assert closed[n] <= F(closed[a] + closed[n - a]), (n, a)
	assert (closed[:len_t + 1] <= convex[:len_t + 1]).all() and closed[2] < convex[2]
	want = convex.copy()
	for n in range(2, len_t + 1):
		for a in range(1, n):
			want[n] = min(want[n], F(want[a] + want[n - a]))
	assert (closed[:len_t + 1].view(np.uint32) == want[:len_t + 1].view(np.uint32)).all()
	# no alignment, no gap costs
	given, closed = _closure(driver, convex, len_t, is_align=0)
	assert not given.any() and not closed.any()


def _text(name):
	return open(os.path.join(CSRC, name)).read()


def test_the_key_decoder_has_one_definition():
	units = HOST_UNITS + ("vk_result_host.h", "vk_transport_host.h", "vk_guard.h", "vk_devbuf.h")
	assert [name for name in units if "0x7fffffffu) : ~" in _text(name)] == ["vk_result_host.h"]
	assert "vk_select.hip:17" in _text("vk_result_host.h")   # the encoder it inverts is named
	for name in QUERY_UNITS:   # ... and no unit takes a key apart or makes one by hand
		assert "& 0xffffffffu" not in _text(name) and "1ull << 32" not in _text(name), name


def test_timings_are_stated_in_two_functions():
	fns = {fn for name in HOST_UNITS for fn, _ in _enclosing_functions(_text(name), r"\bhipEventElapsedTime\(")}
	assert fns == {"state_timings", "query_batch_shared_pass"}, fns


def test_the_order_of_a_result_set_has_one_definition():
	for name in QUERY_UNITS:
		text = _text(name)
		assert "vk_host::rank_above(" in text or "vk_host::ranks_before(" in text, name
		# the comparator written out -- `if (a.x != b.x) return a.x > b.x;` -- is gone
		assert not re.findall(r"if \((.+) != (.+)\) return \1 > \2;", text), name
		for line in text.split("\n"):
			if re.search(r"\bstd::(partial_)?sort\(", line):
				assert "ranks_before" in line or "better" in line, (name, line.strip())
	query = _text("vk_query.cpp")
	assert "const auto better = [](const Cand &a, const Cand &b) { return vk_host::ranks_before(" in query
	assert query.count("vk_host::ranks_before(") == 4   # the candidate rounds of the exact transports and of the submatch weight, vk_merge_topk, vk_merge_records
