"""CPU tier: from the selected keys and their tracebacks to a result set (vectorian_amd/csrc/vk_result_host.h) -- the key codec, the
order of a result set, the score of a winner restated from its traceback, the forms of the gap costs.  The header is host-only; a g++
driver (AddressSanitizer, UBSan) runs each rule on inputs from this file, and the answers are held, as bit patterns, against the rule
stated here in numpy float32; likewise the writer of a result set (score_selected, write_result_set, keep_best, write_best).  Text
checks: the three query units carry no copy of these rules of their own and assign no field of a result set."""

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
		# the comparator written out -- `if (a.x != b.x) return a.x > b.x;` -- is gone
		assert not re.findall(r"if \((.+) != (.+)\) return \1 > \2;", text), name
		for line in text.split("\n"):
			if re.search(r"\bstd::(partial_)?sort\(", line):
				assert "ranks_before" in line or "better" in line, (name, line.strip())
		# ... and so are the calls of the rules the writer applies: they are reached through vk_result_host.h's writer alone
		assert "rank_above(" not in text and "reference_score(" not in text, name
	header = _text("vk_result_host.h")
	assert "const auto better = [](const candidate &a, const candidate &b) { return ranks_before(" in header
	assert _text("vk_query.cpp").count("vk_host::ranks_before(") == 2   # vk_merge_topk, vk_merge_records: records of other ranks, by 64-bit slice
	assert "ranks_before(" not in _text("vk_batch.cpp") + _text("vk_longq_host.cpp")


def test_a_result_set_has_one_writer():
	"""outside vk_result_host.h no query unit assigns a field of a result set's arrays"""
	for name in QUERY_UNITS:
		text = _text(name)
		for field in ("score", "sentence", "raw_score", "mapping", "edge_sim"):   # ... through whichever name: out->score[i] = , outs[i].score[j] =
			assert not re.search(r"(->|\.)%s\[[^;=]*\]\s*=[^=]" % field, text), (name, field)
			assert not re.search(r"memcpy\(\s*&?outs?(\[[^\]]*\])?(->|\.)%s\b" % field, text), (name, field)   # ... nor copies into them
		assert "no_flow(" not in text, name
		assert "struct Cand" not in text, name
	header = _text("vk_result_host.h")
	for field in ("score", "sentence", "raw_score"):
		assert len(re.findall(r"out->%s\[i\] = " % field, header)) == 1, field


def test_the_margin_and_the_lowered_floor_have_one_definition():
	units = HOST_UNITS + ("vk_result_host.h", "vk_transport_host.h", "vk_longq_host.h", "vk_route_host.h")
	assert [name for name in units if re.search(r"\bkCanonMargin\s*=", _text(name))] == ["vk_result_host.h"]
	assert [name for name in units if "1e-5f" in _text(name)] == ["vk_result_host.h"]
	assert _text("vk_result_host.h").count("1e-5f") == 1
	assert not [name for name in QUERY_UNITS if "entry_sent.empty() ? " in _text(name)]   # the slice of a row: slice_of_row, vk_internal.h


def test_the_aligner_score_behind_a_score_of_the_batched_pass(driver):
	"""the GEMM path of vk_query_batch: (score / boost of the slice) * len_t, or score * len_t without boosts"""
	rng = np.random.default_rng(23)
	scores = rng.uniform(0.0, 1.0, 40).astype(F)
	slices = rng.integers(0, 50, 40)
	boost = rng.uniform(0.5, 2.0, 50).astype(F)
	for len_t in (1, 7, 16):
		got = driver("unboosted", 40, len_t, 50, *[hexbits(b) for b in boost], *[x for s, g in zip(scores, slices) for x in (hexbits(s), int(g))])
		assert got == [hexbits(F(F(s / boost[g]) * F(len_t))) for s, g in zip(scores, slices)]
		got = driver("unboosted", 40, len_t, 0, *[x for s, g in zip(scores, slices) for x in (hexbits(s), int(g))])
		assert got == [hexbits(F(s * F(len_t))) for s in scores]


def test_the_lowered_floor(driver):
	mins = [F(0.0), F(0.25), F(-0.5), F(1.0), F(3.0), F(-7.5), F(1e-7)]
	out = driver("floor", len(mins), *[hexbits(m) for m in mins])
	assert out[0] == "8"
	assert out[1:] == [hexbits(F(m - F(F(1e-5) * max(F(1.0), abs(m))))) for m in mins]


# ---- the writer: score_selected + write_result_set, keep_best + write_best, held against the statement below

GUARD = 7


def _dump(n_out, capacity, len_t, winners, has_raw, has_map, has_sim):
	"""what the driver prints for arrays of 7s into which `winners` -- (score, slice, raw, map row or None, sim row or None) -- were written"""
	score = [F(GUARD)] * (capacity + 2)
	sent = [GUARD] * (capacity + 2)
	raw = [F(GUARD)] * (capacity + 2)
	mp = [GUARD] * (capacity * len_t + 2)
	sm = [F(GUARD)] * (capacity * len_t + 2)
	for i, (s, g, r, m, e) in enumerate(winners):
		score[1 + i], sent[1 + i] = s, g
		if has_raw:
			raw[1 + i] = r
		if m is not None and has_map:
			mp[1 + i * len_t:1 + (i + 1) * len_t] = [int(x) for x in m]
		if e is not None and has_sim:
			sm[1 + i * len_t:1 + (i + 1) * len_t] = list(e)
	line = lambda xs, f: "".join(f(x) + " " for x in xs)
	return [str(n_out), line(score, hexbits), line(sent, str), line(raw, hexbits), line(mp, str), line(sm, hexbits)]


def _result_case(driver, *, keys, k, min_score=F(-np.inf), listed=False, limit=None, table=None, restate=0, stride=0, len_t=3, rng=None,
		has_raw=True, has_map=True, has_sim=True, flows=True, tagged=False, w=F(0.0), boosted=False, given=None, stated=None, capacity=None):
	"""keys: (score, row) per slot, None = empty.  Runs the driver's `result` rule and holds it against the rule stated here."""
	rng = rng or np.random.default_rng(len(keys) * 131 + stride)
	cap = len(keys)
	n_sel = next((i for i, x in enumerate(keys) if x is None), cap)
	limit = k if limit is None else limit
	capacity = max(limit, 1) if capacity is None else capacity
	rows = [x[1] if x else 0 for x in keys]
	slice_of = (lambda r: table[r]) if table is not None else (lambda r: r)
	numbers = [capacity, len_t, int(has_raw), int(has_map), int(has_sim), int(flows), int(listed), limit, hexbits(min_score)]
	numbers += [len(table), *table] if table is not None else [0]
	numbers += [cap, *[encode(*x) if x else 0 for x in keys], restate, stride]
	val = [F(x[0]) for x in keys[:n_sel]]
	raw = list(val)
	mp = sm = None
	if stride:
		raw_in = rng.uniform(0.0, len_t, cap).astype(F)
		mp = np.where(rng.random((cap, stride)) < 0.6, rng.integers(0, 400, (cap, stride)), -1).astype(np.int16)   # junk beyond len_t included
		sm = rng.random((cap, stride)).astype(F)
		numbers += [*[hexbits(x) for x in raw_in], *[int(x) for x in mp.ravel()], *[hexbits(x) for x in sm.ravel()]]
		raw = list(raw_in[:n_sel])
	if restate == 1:
		tw = rng.uniform(0.1, 2.0, len_t).astype(F) if tagged else None
		total = F(len_t)
		if tagged:
			total = F(0.0)
			for t in tw:
				total = F(total + t)
		boost = rng.uniform(0.5, 2.0, max([slice_of(r) for r in rows] + [0]) + 1).astype(F) if boosted else None
		numbers += [hexbits(total), hexbits(w), *([len_t, *[hexbits(t) for t in tw]] if tagged else [0]), *([len(boost), *[hexbits(b) for b in boost]] if boosted else [0])]
		val = [_reference_score(raw[i], mp[i, :len_t], tw, total, w, boost[slice_of(rows[i])] if boosted else F(1.0)) for i in range(n_sel)]
	elif restate == 2:
		g_raw, g_val = given
		numbers += [*[hexbits(x) for x in g_raw], *[hexbits(x) for x in g_val]]
		raw, val = [F(x) for x in g_raw[:n_sel]], [F(x) for x in g_val[:n_sel]]
	order = list(range(n_sel))
	if restate and not listed:
		order = sorted([i for i in order if val[i] > min_score], key=lambda i: (-float(val[i]), -rows[i]))
	n_out = min(len(order), limit)
	stated = stated(val, rows, order[:n_out]) if stated else []
	numbers += [len(stated), *[hexbits(x) for x in stated]]
	for j, x in enumerate(stated):
		raw[order[j]] = F(x)
	got = driver("result", *numbers)
	assert got[0] == str(n_out)
	assert [int(x) for x in got[1].split()] == order[:n_out]
	rows_go = stride and flows and has_map and has_sim   # flows are written only where the caller asked for them and has both arrays
	winners = [(val[i], slice_of(rows[i]), raw[i], mp[i, :len_t] if rows_go else None, sm[i, :len_t] if rows_go else None) for i in order[:n_out]]
	if not stride and flows and has_map and has_sim:   # the path states no flow
		winners = [(s, g, r, [-1] * len_t, [F(0.0)] * len_t) for s, g, r, _, _ in winners]
	assert got[2:] == _dump(n_out, capacity, len_t, winners, has_raw, has_map, has_sim)
	return order[:n_out], winners


def _keys(rng, n, cap, n_rows=1000):
	"""n selected keys, best first as a selection leaves them, in cap slots"""
	scores = np.sort(rng.uniform(0.0, 1.0, n).astype(F))[::-1]
	rows = rng.permutation(n_rows)[:n]
	return [(F(s), int(r)) for s, r in zip(scores, rows)] + [None] * (cap - n)


@pytest.mark.parametrize("n_sel", [0, 1, 5, 13])   # none, one, k, k + the margin of 8
@pytest.mark.parametrize("stride,len_t", [(16, 5), (64, 17), (80, 65)])
def test_winners_restated_from_their_tracebacks(driver, n_sel, stride, len_t):
	"""alignments with tracebacks (vk_query, long queries, the shared pass): reference_score of every selected slice, the k best above
	min_score in the order of a result set, len_t of a row's `stride` columns copied -- with and without tag weights, a submatch weight (the
	listed slices of vk_query), boosts indexed by slice through a row -> slice table that is not the identity"""
	rng = np.random.default_rng(1000 * n_sel + stride)
	k = 5
	table = [int(x) for x in rng.permutation(1000) * 3 + 1]
	for tagged, w, boosted, tab in [(False, F(0.0), False, None), (True, F(0.0), True, table), (False, F(0.5), True, None), (True, F(0.5), False, table)]:
		_result_case(driver, keys=_keys(rng, n_sel, k + 8), k=k, min_score=F(0.2), table=tab, restate=1, stride=stride, len_t=len_t, rng=rng, tagged=tagged, w=w, boosted=boosted)
		# listed slices: the caller's order, whatever min_score says, n_only of them
		_result_case(driver, keys=_keys(rng, n_sel, n_sel)[::-1], k=k, limit=n_sel, min_score=F(0.9), listed=True, table=tab, restate=1, stride=stride, len_t=len_t, rng=rng,
			tagged=tagged, w=w, boosted=boosted)
	# the caller did not ask for flows it has arrays for / has no arrays: the tracebacks rank the winners and go nowhere
	_result_case(driver, keys=_keys(rng, n_sel, k + 8), k=k, restate=1, stride=stride, len_t=len_t, rng=rng, has_map=False, has_sim=False, has_raw=False)
	_result_case(driver, keys=_keys(rng, n_sel, k + 8), k=k, restate=1, stride=stride, len_t=len_t, rng=rng, flows=False)      # unasked: both arrays stay
	_result_case(driver, keys=_keys(rng, n_sel, k + 8), k=k, restate=1, stride=stride, len_t=len_t, rng=rng, has_sim=False)   # one array only: neither is written


def test_restated_scores_rank_by_score_then_by_the_higher_slice(driver):
	"""ties on the restated score go to the higher slice; a score equal to min_score is out; listed slices ignore both"""
	one, two = F(0.5), F(0.25)
	rows = [10, 400, 7, 12, 900, 3, 5, 6]
	vals = [one, two, one, F(0.75), one, two, F(0.1), F(0.26)]
	keys = [(F(0.9 - 0.1 * i), r) for i, r in enumerate(rows)] + [None, None]
	given = ([F(10 + i) for i in range(10)], vals + [F(99), F(99)])
	order, _ = _result_case(driver, keys=keys, k=6, min_score=two, restate=2, given=given)
	assert order == [3, 4, 0, 2, 7]   # 0.75; the three 0.5s by slice 900, 10, 7; 0.26; the 0.25s equal min_score
	order, _ = _result_case(driver, keys=keys, k=3, min_score=two, restate=2, given=given)
	assert order == [3, 4, 0]
	order, _ = _result_case(driver, keys=keys[:8], k=3, limit=8, min_score=two, listed=True, restate=2, given=(given[0][:8], vals))
	assert order == list(range(8))


def test_scores_as_selected_keep_the_keys_order(driver):
	"""without restating the keys' order is the result's (the span pass, the GEMM pass, vk_query without tracebacks): no ranking, no
	min_score -- the selection applied it -- and the aligner score is the score unless the caller states another"""
	rng = np.random.default_rng(3)
	for n_sel in (0, 1, 5, 13):
		keys = _keys(rng, n_sel, 13)
		_result_case(driver, keys=keys, k=13, min_score=F(0.5), flows=False)                      # the span pass: raw_score = score, flows untouched
		_result_case(driver, keys=keys, k=13, min_score=F(0.5), flows=False, has_raw=False)      # raw_score == nullptr
		_result_case(driver, keys=keys, k=13, flows=True)                                       # flows asked, none stated: no_flow
		_result_case(driver, keys=keys, k=13, flows=True, has_sim=False)                        # ... without both arrays: nothing
		_result_case(driver, keys=keys, k=13, flows=True, has_map=False, has_sim=False)
		# the GEMM pass: the aligner score behind a score -- the boost taken out, the mean over the query's tokens undone; rows are slices
		boost = rng.uniform(0.5, 2.0, 1000).astype(F)
		_result_case(driver, keys=keys, k=13, len_t=7, stated=lambda val, rows, order: [F(F(val[i] / boost[rows[i]]) * F(7)) for i in order])
		# vk_query without tracebacks: the aligner scores gathered from the scoring pass's array, through a row -> slice table
		_result_case(driver, keys=keys, k=13, table=[int(x) for x in rng.permutation(1000) + 5], stated=lambda val, rows, order: [F(rows[i] * 0.5) for i in order])
	# two zeros as keys: -0.0 sorts below +0.0 whatever the rows, and stays there
	_result_case(driver, keys=[(F(0.0), 3), (F(-0.0), 9)], k=2, min_score=F(-1.0))


def test_listed_slices_without_a_score(driver):
	"""the exact transports write -inf for an empty listed slice, the relaxed WMD NaN for one longer than the caller's rows: both stay in
	the caller's order (no ranking meets the NaN), flows stated as none"""
	keys = [(F(1.0), r) for r in (5, 2, 9, 4)]   # key_of_row: any score field
	vals = [F(0.5), F(-np.inf), F(np.nan), F(0.7)]
	raws = [F(2.5), F(-np.inf), F(np.nan), F(3.5)]
	order, winners = _result_case(driver, keys=keys, k=4, limit=4, min_score=F(0.6), listed=True, restate=2, given=(raws, vals), table=[0, 10, 20, 30, 40, 50, 60, 70, 80, 90])
	assert order == [0, 1, 2, 3] and [g for _, g, _, _, _ in winners] == [50, 20, 90, 40]


def _keep_best_case(driver, rounds, k, min_score, len_t, table=None, flows=True, has_raw=True, has_map=True, has_sim=True):
	"""rounds: lists of (val, raw, row, map row or None, sim row or None)"""
	capacity = k
	numbers = [capacity, len_t, int(has_raw), int(has_map), int(has_sim), int(flows), k, hexbits(min_score)]
	numbers += [len(table), *table] if table is not None else [0]
	numbers.append(len(rounds))
	best, kept = [], []
	for rnd in rounds:
		numbers.append(len(rnd))
		for val, raw, row, m, e in rnd:
			numbers += [hexbits(val), hexbits(raw), row, 0 if m is None else len_t, *([] if m is None else [int(x) for x in m]), *([] if e is None else [hexbits(x) for x in e])]
		best = sorted(best + [cd for cd in rnd if cd[0] > min_score], key=lambda cd: (-float(cd[0]), -cd[2]))[:k]
		kept.append([cd[2] for cd in best])
	got = driver("keep_best", *numbers)
	assert [[int(x) for x in line.split()] for line in got[:len(rounds)]] == kept
	rows_go = flows and has_map and has_sim
	winners = [(val, table[row] if table is not None else row, raw, m if rows_go else None, e if rows_go else None) for val, raw, row, m, e in best]
	if rows_go:   # a candidate without a traceback (the transports): no flow stated
		winners = [(s, g, r, [-1] * len_t if m is None else m, [F(0.0)] * len_t if e is None else e) for s, g, r, m, e in winners]
	assert got[len(rounds):] == _dump(len(best), capacity, len_t, winners, has_raw, has_map, has_sim)
	return kept


def test_keep_best_over_three_rounds(driver):
	"""the candidate rounds of the exact transports (no tracebacks) and of the submatch weight (tracebacks): three rounds whose union
	exceeds k, duplicate scores (the higher row first), a candidate equal to min_score (out)"""
	rng = np.random.default_rng(17)
	len_t, k, min_score = 4, 5, F(0.25)
	vals = [[F(0.5), F(0.25), F(0.3), F(0.1)], [F(0.5), F(0.9), F(0.5), F(0.26)], [F(0.25), F(0.6), F(0.9), F(0.2), F(0.5)]]
	rows = [[4, 8, 15, 16], [23, 42, 1, 2], [3, 5, 6, 7, 99]]
	for traced in (False, True):
		rounds = [[(v, F(10 * v), r, rng.integers(-1, 50, len_t).astype(np.int16) if traced else None, rng.random(len_t).astype(F) if traced else None)
			for v, r in zip(vs, rs)] for vs, rs in zip(vals, rows)]
		kept = _keep_best_case(driver, rounds, k, min_score, len_t)
		assert kept == [[4, 15], [42, 23, 4, 1, 15], [42, 6, 5, 99, 23]]
		_keep_best_case(driver, rounds, k, min_score, len_t, table=[int(x) for x in np.arange(100) * 2 + 1], flows=False)   # flows unasked: the arrays stay
		_keep_best_case(driver, rounds, k, min_score, len_t, has_raw=False, has_sim=False)   # flows asked without both arrays: nothing
	_keep_best_case(driver, [[], [], []], k, min_score, len_t)
