"""-m gpu: the 6-bit bound pass against the exact pass it stands in for, by the claims of tests/test_gpu_bound_pass.py.
Every case runs the same query on two handles of the same vectors -- one finalized and queried with VK_BOUND_PASS=force
VK_BOUND_BITS=6 (an E2M3 shadow, MODE 8 and the two rounds), one with VK_BOUND_PASS=off -- and asserts
  (a) the two result sets are the same arrays: score and aligner score as bit patterns, sentence, mapping, edge similarities;
  (b) the bound of every non-empty slice is >= the exact pass's score of it;
  (c) last_scores() after the pruned query equals the exact pass's, bit for bit;
  (d) the counters say a bound pass ran on a 6-bit shadow and did not fall back -- wherever round2_limit, the most slices round 2 can
      hold by the exact scores and delta_6, is within max(n / 16, 1024), the line beyond which the library runs the full pass instead;
      where the limit lies beyond that line either outcome is right and (a) .. (c) hold all the same (delta_6 is four times the 8-bit
      delta, and a short query over a few thousand slices has more than n / 16 of them within 2 delta_6 of its 18th best).  The
      module prints how many cases took each branch when it ends.  10-token queries under local alignment on the 4,000 x 32 shape
      assert no fallback whatever the limit says: the simulation's largest round 2 at that size, 651, is below the line of 1,024;
  (e) bound - exact <= delta_6 and round 2 <= round2_limit(delta_6), delta_6 from the numpy restatement of the E2M3 quantizer
      (tests/bound6_cases.py).
The 1 % cap on round 2 of 10-token queries that the 8-bit test asserts on the 4,000 x 32 shape is NOT asserted here: the CPU
simulation (tools/sim_bound_bits.py --slices 4000 --chunk 4000 --queries 16) gives 30 .. 122 slices for planted and 143 .. 651 for random
queries under E2M3 at that size (int8: 20 .. 46), 0.8 .. 16 %; the count hardly grows with the corpus, so 1 % is a claim
about 50,000 slices and more, which profiles/bound_fp6_sim.json and the benchmark's own counters record.
Shapes: 4,000 x 32 tokens; 3,000 slices of 1 .. 64 tokens with empty ones (both register-history depths); 37 slices of 1 .. 3 tokens.
Widths 289, 303 and 304 build a 6-bit shadow, 288 and 305 none.  Without VK_BOUND_BITS, force keeps the 8-bit shadow."""

import ctypes as C
import threading

import numpy as np
import pytest

import bound6_cases as b6
import bound_cases as bc
from bound_cases import case_queries, corpus_of as _corpus, ragged_with_empties, same_results, state
from vectorian_amd import synth

pytestmark = pytest.mark.gpu

D, V = 300, 50_000
EXP5 = ("table", (1 - 2.0 ** (-np.arange(0, 65) / 5)).astype(np.float32))
GAPS = {"linear": (0.1, 0.1), "affine": (("affine", 0.2, 0.05), ("affine", 0.2, 0.05)), "exp5": (EXP5, EXP5)}
TILE6, TILE8 = 3968, 5248


def _Env(mode, bits="6"):
	"""VK_BOUND_PASS and VK_BOUND_BITS for the duration of a block (the library reads them at finalize and per query)"""
	return bc.Env(VK_BOUND_PASS=mode, VK_BOUND_BITS=bits)


def bits_of(hip, c):
	lib = hip.lib()
	lib.vk_bound_pass_bits.restype = C.c_int
	lib.vk_bound_pass_bits.argtypes = [C.c_void_p, C.c_void_p]
	out = C.c_int64(-1)
	with c.lock:
		hip._check(lib.vk_bound_pass_bits(c._h, C.byref(out)))
	return out.value


class Pair(bc.Pair):
	"""the same vectors twice: `forced` has a 6-bit shadow, `exact` has none"""

	def __init__(self, hip, corpus, X=None, off=None):
		super().__init__(hip, _Env, corpus, X, off)
		tiles = self.X.shape[0] // 16
		extra = self.forced.device_bytes - self.exact.device_bytes
		# the shadow is counted: 3,968 bytes per tile of 16 tokens (a few tiles of padding; far from the 8-bit shadow's 5,248)
		assert bits_of(hip, self.forced) == 6 and bits_of(hip, self.exact) == 0
		assert tiles * TILE6 <= extra <= (tiles + 8) * TILE6 + 4096, (extra, tiles)
		self.terms = b6.corpus_terms(b6.stored(self.X))


BRANCHES = {"asserted no fallback": 0, "either outcome allowed": 0, "fell back where allowed": 0}


@pytest.fixture(scope="module", autouse=True)
def branches_taken():
	yield
	print(f"\nclaim (d): {BRANCHES}")


def check(hip, pair, qv, expect_fallback=False, strict=False, **kw):
	"""one query both ways: (a) .. (e) of the module's text; returns the counters"""
	with _Env("force"):
		got = pair.forced.query(qv, **kw)
		ub, cnt = state(hip, pair.forced)
		mine = pair.forced.last_scores()
	with _Env("off"):
		ref = pair.exact.query(qv, **kw)
		_, cnt_off = state(hip, pair.exact, bounds=False)
		full = pair.exact.last_scores()
	some = np.isfinite(full) & np.isfinite(ub)
	slack = (ub[some] - full[some]).max() if some.any() else 0.0
	print(f"n {pair.n} len_t {len(qv)} k {kw.get('max_matches')} locality {kw.get('locality')}: round 1 {cnt[1]}, round 2 {cnt[2]}, fell back {cnt[3]}, "
		f"bound - exact: max {slack:.5f}")
	assert cnt_off[0] == 0
	assert cnt[0] == 1, cnt                                       # (d)
	delta = b6.delta6(pair.terms, b6.stored(qv))
	limit = b6.round2_limit(delta, full, kw["max_matches"], pair.n, kw.get("min_score", 0.0)) if kw.get("boost") is None else None
	if expect_fallback:
		assert cnt[3] == 1, cnt
	elif strict or limit is None or limit <= max(pair.n // 16, 1024):
		BRANCHES["asserted no fallback"] += 1
		assert cnt[3] == 0, (cnt, limit)
	else:
		BRANCHES["either outcome allowed"] += 1
		BRANCHES["fell back where allowed"] += int(cnt[3])
	same_results(got, ref)                                        # (a)
	nonempty = np.diff(pair.off) > 0
	assert (ub[nonempty] >= full[nonempty]).all(), (ub[nonempty] - full[nonempty]).min()   # (b)
	assert (mine.view(np.uint32) == full.view(np.uint32)).all()   # (c)
	if cnt[3] == 0 and limit is not None:
		print(f"  round 2 {cnt[2]} <= {limit}, delta_6 {delta:.5f}")
		assert some.any() and slack <= delta, (slack, delta)        # (e)
		assert cnt[2] <= limit, (cnt, limit)
	return cnt


@pytest.fixture(scope="module")
def uniform(hip):
	p = Pair(hip, synth.make_contextual_corpus(4000, 32, 32, V, D))
	yield p
	p.close()


@pytest.fixture(scope="module")
def ragged(hip):
	p = Pair(hip, ragged_with_empties(D, 3000, seed=41))
	yield p
	p.close()


@pytest.fixture(scope="module")
def tiny(hip):
	p = Pair(hip, synth.make_contextual_corpus(37, 1, 3, V, D, seed=43))
	yield p
	p.close()


@pytest.mark.parametrize("gap", sorted(GAPS))
@pytest.mark.parametrize("shape", ("uniform", "ragged", "tiny"))
def test_pruned_query_is_the_exact_query(hip, request, shape, gap):
	pair = request.getfixturevalue(shape)
	gs, gt = GAPS[gap]
	for len_t in (1, 4, 10, 12, 16):
		for qv in case_queries(pair.corpus, len_t):
			for locality in (0, 1, 2):
				for k in (1, 10):
					check(hip, pair, qv, strict=shape == "uniform" and len_t == 10 and locality == 0,
						locality=locality, gap_s=gs, gap_t=gt, max_matches=k, min_score=0.0 if locality == 0 else -1e9)


@pytest.mark.parametrize("d", (289, 303, 304))
def test_widths_that_build_a_6bit_shadow(hip, d):
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
	corpus = ragged_with_empties(d, 1500, seed=50 + d)
	with _Env("off"):
		exact = _corpus(hip, corpus["X"], corpus["sent_off"])
	with _Env("force"):
		forced = _corpus(hip, corpus["X"], corpus["sent_off"])
	try:
		assert forced.device_bytes == exact.device_bytes and bits_of(hip, forced) == 0
		for qv in case_queries(corpus, 10):
			kw = dict(locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10)
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
	rng = np.random.default_rng(2)
	qv = (uniform.corpus["E"][0] + 0.05 * rng.standard_normal(D)).astype(np.float32)[None, :]
	assert (uniform.corpus["tok_id"] == 0).mean() > 0.05
	for k in (1, 10):
		cnt = check(hip, uniform, qv, expect_fallback=True, locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=k)
		assert cnt[2] > uniform.n // 2


def test_boost_and_min_score(hip, uniform):
	qv = synth.make_queries(uniform.corpus, 1, 10, seed=7)[0]["vectors"]
	rng = np.random.default_rng(5)
	boost = rng.uniform(0.0, 2.0, size=uniform.n).astype(np.float32)
	boost[::97] = 0.0
	check(hip, uniform, qv, locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10, boost=boost)
	check(hip, uniform, qv, locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10, min_score=0.3)


def test_a_view_beside_its_parent(hip, uniform):
	qs = [q["vectors"] for q in synth.make_queries(uniform.corpus, 8, 10, seed=77)]
	kw = dict(locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10)
	with _Env("force"):
		alone = [uniform.forced.query(q, **kw) for q in qs]
		handles = [uniform.forced, uniform.forced.view()]
		assert bits_of(hip, handles[1]) == 6
		before = [int(state(hip, h, bounds=False)[1][4]) for h in handles]
		out = [[None] * len(qs) for _ in handles]
		fell = [0, 0]

		def work(i):
			for j, q in enumerate(qs):
				out[i][j] = handles[i].query(q, **kw)
				fell[i] += int(state(hip, handles[i], bounds=False)[1][3])
		threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
		for t in threads:
			t.start()
		for t in threads:
			t.join()
		after = [int(state(hip, h, bounds=False)[1][4]) for h in handles]
		handles[1].close()
	for i in range(2):
		assert after[i] - before[i] == len(qs) and fell[i] == 0    # every query of either handle took the bound pass
		for j in range(len(qs)):
			same_results(out[i][j], alone[j])


def test_force_without_bits_keeps_the_8bit_shadow(hip):
	corpus = synth.make_contextual_corpus(500, 32, 32, V, D, seed=8)
	with _Env("off"):
		exact = _corpus(hip, corpus["X"], corpus["sent_off"])
	with _Env("force", bits=None):
		unset = _corpus(hip, corpus["X"], corpus["sent_off"])
	with _Env("force", bits="8"):
		eight = _corpus(hip, corpus["X"], corpus["sent_off"])
	try:
		assert bits_of(hip, unset) == 8 and bits_of(hip, eight) == 8
		assert unset.device_bytes == eight.device_bytes
		assert unset.device_bytes - exact.device_bytes >= (corpus["X"].shape[0] // 16) * TILE8
		qv = synth.make_queries(corpus, 1, 10, seed=3)[0]["vectors"]
		kw = dict(locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10)
		with _Env("force", bits=None):
			got = unset.query(qv, **kw)
			assert state(hip, unset, bounds=False)[1][0] == 1
		with _Env("off"):
			same_results(got, exact.query(qv, **kw))
	finally:
		for c in (exact, unset, eight):
			c.close()
