"""-m gpu: the 8-bit bound pass against the exact pass it stands in for.  Every case runs the same query on two handles of the
same vectors -- one finalized and queried with VK_BOUND_PASS=force (a shadow, the bound pass and its two rounds), one finalized with
VK_BOUND_PASS=off (no shadow: the exact pass over every slice) -- and asserts
  (a) the two result sets are the same arrays: score and aligner score as bit patterns, sentence, mapping, edge similarities;
  (b) the bound of every non-empty slice is >= the exact pass's score of it (the correctness claim of the whole path);
  (c) last_scores() after the pruned query equals the exact pass's, bit for bit;
  (d) the counters say the bound pass ran and did not fall back to the full pass (unless the case is about the fallback).
Shapes: 4,000 x 32 tokens (whole tiles, 1,000 groups: four workgroup rounds), 3,000 slices of 1..64 tokens with empty ones among them
(slices across tile borders, both register-history depths), 37 slices of 1..3 tokens (fewer slices than candidates of round 1).  All
300-d, the compile-time form of the bound kernel; its width edges on a corpus of their own: 289, 303 and 304 features (15, one and no
padded feature in the last half block of the exact tiles; the shadow's fifth K-step of 64 holds 33, 47 and 48 live bytes) through (a) .. (e),
and 288 and 305 features, where no shadow may exist.  The lane map of the 8-bit MFMA is checked with exact integers.
  (e) The bound exceeds the exact score by no more than the derived delta, and round 2 holds no more slices than follows from the exact
scores and delta (round2_limit): every case of every shape, so that a bound that got worse (a larger gamma, a coarser quantizer) fails here; on the 4,000 x 32 shape 10-token queries at
k <= 10 also stay within 1 % of the slices.
One-token queries: only the word drawn from the vocabulary runs through (a) .. (e) -- the copied corpus token is a frequent word and falls
back, which test_a_frequent_word_falls_back states; so no one-token query of a word that occurs in the corpus is tested WITHOUT a
fallback, a narrower length-1 case than a query copied from the corpus would be."""

import ctypes as C
import threading

import numpy as np
import pytest

import bound_cases as bc
from bound_cases import case_queries, corpus_of as _corpus, ragged_with_empties, same_results, state
from vectorian_amd import synth

pytestmark = pytest.mark.gpu

D, V = 300, 50_000
EXP5 = ("table", (1 - 2.0 ** (-np.arange(0, 65) / 5)).astype(np.float32))
GAPS = {"linear": (0.1, 0.1), "affine": (("affine", 0.2, 0.05), ("affine", 0.2, 0.05)), "exp5": (EXP5, EXP5)}


def _Env(value):
	"""VK_BOUND_PASS for the duration of a block (the library reads it at finalize and per query)"""
	return bc.Env(VK_BOUND_PASS=value)


class Pair(bc.Pair):
	"""the same vectors twice: `forced` has a shadow, `exact` has none"""

	def __init__(self, hip, corpus, X=None, off=None):
		super().__init__(hip, _Env, corpus, X, off)
		# the shadow is counted: 5 KiB + 128 bytes per tile of 16 tokens beside 9.5 KiB
		assert self.forced.device_bytes - self.exact.device_bytes >= (self.X.shape[0] // 16) * (5 * 1024 + 128)


def round2_limit(pair, qv, full, k, min_score):
	"""(delta, the most slices round 2 can hold) with the 300-d forms' d_pad = 320 in gamma (bound_cases.round2_limit8)"""
	return bc.round2_limit8(pair, qv, full, k, min_score, 320)


def check(hip, pair, qv, expect_fallback=False, **kw):
	"""one query both ways: (a) .. (d) of the module's text; returns the counters"""
	with _Env("force"):
		got = pair.forced.query(qv, **kw)
		ub, cnt = state(hip, pair.forced)
		mine = pair.forced.last_scores()
	with _Env("off"):
		ref = pair.exact.query(qv, **kw)
		_, cnt_off = state(hip, pair.exact, bounds=False)
		full = pair.exact.last_scores()
	some = np.isfinite(full) & np.isfinite(ub)
	print(f"n {pair.n} len_t {len(qv)} k {kw.get('max_matches')} locality {kw.get('locality')}: round 1 {cnt[1]}, round 2 {cnt[2]}, fell back {cnt[3]}, "
		f"bound - exact: max {(ub[some] - full[some]).max() if some.any() else 0.0:.5f}")
	assert cnt_off[0] == 0                                        # no shadow, no bound pass
	assert cnt[0] == 1 and cnt[3] == (1 if expect_fallback else 0), cnt   # (d)
	same_results(got, ref)                                        # (a)
	nonempty = np.diff(pair.off) > 0
	assert (ub[nonempty] >= full[nonempty]).all(), (ub[nonempty] - full[nonempty]).min()   # (b)
	assert (mine.view(np.uint32) == full.view(np.uint32)).all()   # (c)
	if not expect_fallback and kw.get("boost") is None:
		delta, limit = round2_limit(pair, qv, full, kw["max_matches"], kw.get("min_score", 0.0))
		print(f"  round 2 {cnt[2]} <= {limit}, delta {delta:.5f}")
		assert some.any() and (ub[some] - full[some]).max() <= delta, ((ub[some] - full[some]).max(), delta)   # (e): the bound is as tight as derived
		assert cnt[2] <= limit, (cnt, limit)                        # (e): ... and round 2 as small
	return cnt


@pytest.fixture(scope="module")
def uniform(hip):
	p = Pair(hip, synth.make_contextual_corpus(4000, 32, 32, V, D))
	yield p
	p.close()


@pytest.fixture(scope="module")
def ragged(hip):
	corpus = synth.make_contextual_corpus(2995, 1, 64, V, D, seed=41)
	off = corpus["sent_off"]
	at = np.array([0, 7, 1500, 2994, 2995])                      # empty slices: first, inside a group, last
	corpus["sent_off"] = np.insert(off, at, off[at])
	assert len(corpus["sent_off"]) - 1 == 3000 and (np.diff(corpus["sent_off"]) == 0).sum() == 5
	p = Pair(hip, corpus)
	yield p
	p.close()


@pytest.fixture(scope="module")
def tiny(hip):
	p = Pair(hip, synth.make_contextual_corpus(37, 1, 3, V, D, seed=43))
	yield p
	p.close()


@pytest.mark.parametrize("gap", sorted(GAPS))
@pytest.mark.parametrize("len_t", (1, 4, 10, 16))
@pytest.mark.parametrize("shape", ("uniform", "ragged", "tiny"))
def test_pruned_query_is_the_exact_query(hip, request, shape, len_t, gap):
	"""every case through (a) .. (e); 10-token queries at k <= 10 on the 4,000 x 32 shape also within the 1 % of the simulation that
	predicted it (at k = 100 the 108 candidates there must be are 2.7 % already; shorter queries: DESIGN 11.6)"""
	pair = request.getfixturevalue(shape)
	gs, gt = GAPS[gap]
	for qv in case_queries(pair.corpus, len_t):
		for locality in (0, 1, 2):
			for k in (1, 10, 100):
				# (global and semiglobal scores are mostly negative: every slice takes part)
				cnt = check(hip, pair, qv, locality=locality, gap_s=gs, gap_t=gt, max_matches=k, min_score=0.0 if locality == 0 else -1e9)
				if shape == "uniform" and len_t == 10 and k <= 10:
					assert cnt[2] <= pair.n // 100, cnt


@pytest.mark.parametrize("d", (289, 303, 304))
def test_width_edges_of_the_shadow(hip, d):
	"""every width that builds a shadow shares the 300-d forms (d_pad = 304): the widest, with no padding in the half block, the
	narrowest, with 15 padded features and d % 4 == 1, and one short of the widest -- every case through (a) .. (e)"""
	pair = Pair(hip, ragged_with_empties(d, 1500, seed=50 + d))
	try:
		for len_t in (4, 16):
			for qv in case_queries(pair.corpus, len_t):
				for gap in sorted(GAPS):
					gs, gt = GAPS[gap]
					for locality in (0, 1):
						check(hip, pair, qv, locality=locality, gap_s=gs, gap_t=gt, max_matches=10, min_score=0.0 if locality == 0 else -1e9)
	finally:
		pair.close()


@pytest.mark.parametrize("d", (288, 305))
def test_no_shadow_beside_its_widths(hip, d):
	"""d_pad = 288 and d_pad = 320: VK_BOUND_PASS=force builds no shadow (the same bytes on the device as with `off`), no bound pass
	runs, and the results are the exact pass's"""
	corpus = ragged_with_empties(d, 1500, seed=50 + d)
	with _Env("off"):
		exact = _corpus(hip, corpus["X"], corpus["sent_off"])
	with _Env("force"):
		forced = _corpus(hip, corpus["X"], corpus["sent_off"])
	try:
		assert forced.device_bytes == exact.device_bytes
		for len_t in (4, 16):
			for qv in case_queries(corpus, len_t):
				for gap in sorted(GAPS):
					gs, gt = GAPS[gap]
					kw = dict(locality=0, gap_s=gs, gap_t=gt, max_matches=10)
					with _Env("force"):
						got = forced.query(qv, **kw)
						assert state(hip, forced, bounds=False)[1][0] == 0
					with _Env("off"):
						ref = exact.query(qv, **kw)
					same_results(got, ref)
	finally:
		forced.close()
		exact.close()


def test_a_frequent_word_falls_back(hip, uniform):
	"""a one-token query of the corpus's most frequent word: nearly every slice holds the word, the bounds separate nothing -- the full
	pass runs (and says so), the results are the exact pass's"""
	rng = np.random.default_rng(2)
	qv = (uniform.corpus["E"][0] + 0.05 * rng.standard_normal(D)).astype(np.float32)[None, :]
	assert (uniform.corpus["tok_id"] == 0).mean() > 0.05
	for k in (1, 10, 100):
		cnt = check(hip, uniform, qv, expect_fallback=True, locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=k)
		assert cnt[2] > uniform.n // 2


def test_boost_and_min_score(hip, uniform):
	qv = synth.make_queries(uniform.corpus, 1, 10, seed=7)[0]["vectors"]
	rng = np.random.default_rng(5)
	boost = rng.uniform(0.0, 2.0, size=uniform.n).astype(np.float32)
	boost[::97] = 0.0
	check(hip, uniform, qv, locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10, boost=boost)
	check(hip, uniform, qv, locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10, min_score=0.3)
	# a negative boost turns the order of the scores around: no bound pass, the exact pass as ever
	boost[5] = -1.0
	with _Env("force"):
		got = uniform.forced.query(qv, locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10, boost=boost)
		assert state(hip, uniform.forced, bounds=False)[1][0] == 0
	same_results(got, uniform.exact.query(qv, locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10, boost=boost))


def test_identical_sentences_fall_back(hip):
	"""2,000 copies of one sentence: every bound ties, the bounds separate nothing -- the full pass runs, and says so"""
	base = synth.make_contextual_corpus(1, 32, 32, V, D, seed=3)
	pair = Pair(hip, base, X=np.tile(base["X"], (2000, 1)), off=np.arange(2001, dtype=np.int64) * 32)
	qv = synth.make_queries(base, 1, 10, seed=1)[0]["vectors"]
	cnt = check(hip, pair, qv, expect_fallback=True, locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10)
	assert cnt[2] == 2000
	pair.close()


def test_ties_at_the_kth_place(hip):
	"""blocks of eight copies of a sentence: the k-th place falls inside a block of equal scores"""
	base = synth.make_contextual_corpus(500, 32, 32, V, D, seed=9)
	X = np.repeat(base["X"].reshape(500, 32, D), 8, axis=0).reshape(-1, D)
	pair = Pair(hip, base, X=X, off=np.arange(4001, dtype=np.int64) * 32)
	for len_t, k in ((10, 10), (10, 3), (4, 100), (16, 1)):
		qv = synth.make_queries(base, 1, len_t, seed=len_t)[0]["vectors"]
		check(hip, pair, qv, locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=k)
		check(hip, pair, qv, locality=0, gap_s=0.1, gap_t=0.1, max_matches=k)
	pair.close()


def test_two_views_from_two_threads(hip, uniform):
	qs = [q["vectors"] for q in synth.make_queries(uniform.corpus, 20, 10, seed=77)]
	kw = dict(locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10)
	with _Env("force"):
		alone = [uniform.forced.query(q, **kw) for q in qs]
		views = [uniform.forced.view(), uniform.forced.view()]
		out = [[None] * len(qs) for _ in views]
		fell = [0, 0]

		def work(i):
			for j, q in enumerate(qs):
				out[i][j] = views[i].query(q, **kw)
				fell[i] += int(state(hip, views[i], bounds=False)[1][3])
		threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
		for t in threads:
			t.start()
		for t in threads:
			t.join()
		counters = [state(hip, v, bounds=False)[1] for v in views]
		for v in views:
			v.close()
	for i in range(2):
		assert counters[i][4] == len(qs) and fell[i] == 0, counters[i]   # every query of a view took the bound pass
		for j in range(len(qs)):
			same_results(out[i][j], alone[j])


def test_lane_map_of_the_8bit_mfma(hip):
	"""one tile and one query of distinct small integers through v_mfma_i32_16x16x64_i8, packed as the shadow packs them: the product is
	numpy's integer product exactly"""
	lib = hip.lib()
	lib.vk_i8_tile_probe.restype = C.c_int
	lib.vk_i8_tile_probe.argtypes = [C.c_void_p] * 3
	rng = np.random.default_rng(1)
	for q, x in (
		((np.arange(1024).reshape(16, 64) % 251 - 125).astype(np.int8), ((np.arange(1024).reshape(16, 64) * 7 + 3) % 241 - 120).astype(np.int8)),
		(rng.integers(-127, 128, size=(16, 64)).astype(np.int8), rng.integers(-127, 128, size=(16, 64)).astype(np.int8)),
		(np.eye(16, 64, k=5, dtype=np.int8) * 3, (np.arange(1024).reshape(16, 64) % 127).astype(np.int8)),
	):
		q, x = np.ascontiguousarray(q), np.ascontiguousarray(x)
		out = np.zeros((16, 16), dtype=np.int32)
		hip._check(lib.vk_i8_tile_probe(q.ctypes.data, x.ctypes.data, out.ctypes.data))
		assert (out == q.astype(np.int32) @ x.astype(np.int32).T).all()
