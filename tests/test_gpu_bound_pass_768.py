"""-m gpu: the 8-bit bound pass over corpora whose rows pad to 768 features (twelve K-steps of 64 int8, 12,416 bytes per shadow
tile) against the exact pass it stands in for -- what tests/test_gpu_bound_pass.py asserts at 300-d, here at 753 .. 768.  Every case
runs the same query on two handles of the same vectors, one finalized and queried with VK_BOUND_PASS=force, one with VK_BOUND_PASS=off:
  (a) the two result sets are the same arrays, bit for bit;
  (b) the bound of every non-empty slice is >= the exact pass's score of it;
  (c) last_scores() after the pruned query equals the exact pass's, bit for bit;
  (d) the bound pass ran and did not fall back (10- and 16-token queries never; the one-token query of a frequent word does, and is
      asserted to);
  (e) bound - exact <= delta, and round 2 holds no more slices than follows from the exact scores and delta -- delta as in the 300-d
      module with this corpus's own d_pad in gamma: 2 x 768 x 2^-24 a_q X + 2e-6.
Shapes: 2,000 slices of 1 .. 64 tokens with five empty ones (tile borders, both register-history depths, two workgroup rounds), 1,500
slices of 32 tokens.  Widths: 753 (the narrowest row of the form, d % 4 == 1), 760, 767 and 768 -- the last K-step's last quarter
holds 1, 8, 15 and 16 features; every width of the form has all four quarters of the last K-step live (704 + 48 < 753), so the partial
fetch of tests/test_gpu_bound_live_bytes.py never drops a load here -- and 752 / 769 (d_pad 752 / 784), where no shadow may exist.
The one-token query that must not fall back is a word that occurs in at most five tokens of the corpus."""

import threading

import numpy as np
import pytest

import bound_cases as bc
from bound_cases import case_queries, corpus_of as _corpus, ragged_with_empties, same_results, state
from test_gpu_bound_pass import EXP5, _Env
from vectorian_amd import synth

pytestmark = pytest.mark.gpu

V = 50_000
D_PAD = 768
TILE8 = 12 * 1024 + 128
GAPS = {"linear": (0.1, 0.1), "exp5": (EXP5, EXP5)}


class Pair(bc.Pair):
	"""the same vectors twice: `forced` has a shadow, `exact` has none"""

	def __init__(self, hip, corpus):
		super().__init__(hip, _Env, corpus)
		# the shadow is counted: 12 KiB + 128 bytes per tile of 16 tokens beside 24 KiB
		assert self.forced.device_bytes - self.exact.device_bytes >= (self.X.shape[0] // 16) * TILE8


def round2_limit(pair, qv, full, k, min_score):
	"""(delta, the most slices round 2 can hold): round2_limit of the 300-d module with d_pad = 768 in gamma"""
	return bc.round2_limit8(pair, qv, full, k, min_score, D_PAD)


def check(hip, pair, qv, expect_fallback=False, **kw):
	"""one query both ways: (a) .. (e); returns the counters"""
	with _Env("force"):
		got = pair.forced.query(qv, **kw)
		ub, cnt = state(hip, pair.forced)
		mine = pair.forced.last_scores()
	with _Env("off"):
		ref = pair.exact.query(qv, **kw)
		_, cnt_off = state(hip, pair.exact, bounds=False)
		full = pair.exact.last_scores()
	some = np.isfinite(full) & np.isfinite(ub)
	print(f"d {pair.X.shape[1]} n {pair.n} len_t {len(qv)} locality {kw.get('locality')}: round 1 {cnt[1]}, round 2 {cnt[2]}, fell back {cnt[3]}, "
		f"bound - exact: max {(ub[some] - full[some]).max() if some.any() else 0.0:.5f}")
	assert cnt_off[0] == 0
	assert cnt[0] == 1 and cnt[3] == (1 if expect_fallback else 0), cnt   # (d)
	same_results(got, ref)                                        # (a)
	nonempty = np.diff(pair.off) > 0
	assert (ub[nonempty] >= full[nonempty]).all(), (ub[nonempty] - full[nonempty]).min()   # (b)
	assert (mine.view(np.uint32) == full.view(np.uint32)).all()   # (c)
	if not expect_fallback:
		delta, limit = round2_limit(pair, qv, full, kw["max_matches"], kw.get("min_score", 0.0))
		print(f"  round 2 {cnt[2]} <= {limit}, delta {delta:.5f}")
		assert some.any() and (ub[some] - full[some]).max() <= delta, ((ub[some] - full[some]).max(), delta)   # (e)
		assert cnt[2] <= limit, (cnt, limit)
	return cnt


SHAPES = {"ragged753": (753, None), "ragged760": (760, None), "ragged767": (767, None), "ragged768": (768, None), "uniform768": (768, 32)}


@pytest.fixture(scope="module", params=sorted(SHAPES))
def pair(hip, request):
	d, fixed = SHAPES[request.param]
	corpus = synth.make_contextual_corpus(1500, fixed, fixed, V, d, seed=61) if fixed else ragged_with_empties(d, 2000, seed=50 + d)
	p = Pair(hip, corpus)
	yield p
	p.close()


def rare_word(corpus, seed):
	"""a one-token query of a word that occurs in the corpus, in at most five tokens"""
	counts = np.bincount(corpus["tok_id"], minlength=V)
	ids = np.flatnonzero((counts >= 1) & (counts <= 5))
	rng = np.random.default_rng(seed)
	w = int(ids[rng.integers(0, len(ids))])
	return (corpus["E"][w] + 0.05 * rng.standard_normal(corpus["E"].shape[1])).astype(np.float32)[None, :]


@pytest.mark.parametrize("gap", sorted(GAPS))
@pytest.mark.parametrize("len_t", (1, 10, 16))
def test_pruned_query_is_the_exact_query(hip, pair, len_t, gap):
	"""(a) .. (e), no fallback: local and global alignment, top 10"""
	gs, gt = GAPS[gap]
	queries = [rare_word(pair.corpus, 5)] if len_t == 1 else case_queries(pair.corpus, len_t)
	for qv in queries:
		for locality in (0, 1):
			check(hip, pair, qv, locality=locality, gap_s=gs, gap_t=gt, max_matches=10, min_score=0.0 if locality == 0 else -1e9)


def test_affine_gaps_and_eight_columns(hip):
	"""the forms the cases above do not reach: affine gaps (4, 8, 12 and 16 query columns) and queries of 5 and 8 tokens, which pad to
	eight columns, under every gap kind -- one ragged shape, (a) .. (e), no fallback"""
	affine = (("affine", 0.2, 0.05), ("affine", 0.2, 0.05))
	p = Pair(hip, ragged_with_empties(768, 2000, seed=97))
	try:
		for len_t in (4, 5, 8, 10, 16):
			for gs, gt in [affine] + ([GAPS["linear"], GAPS["exp5"]] if len_t in (5, 8) else []):
				for qv in case_queries(p.corpus, len_t):
					for locality in (0, 1):
						check(hip, p, qv, locality=locality, gap_s=gs, gap_t=gt, max_matches=10, min_score=0.0 if locality == 0 else -1e9)
	finally:
		p.close()


def test_a_frequent_word_falls_back(hip, pair):
	"""a one-token query of the corpus's most frequent word: most slices hold it and tie within the quantization error -- the full
	pass runs, and says so; the results are the exact pass's"""
	rng = np.random.default_rng(2)
	qv = (pair.corpus["E"][0] + 0.05 * rng.standard_normal(pair.X.shape[1])).astype(np.float32)[None, :]
	seen = np.concatenate([[0], np.cumsum(pair.corpus["tok_id"] == 0)])
	holds = seen[pair.off[1:]] > seen[pair.off[:-1]]
	assert holds.sum() > max(pair.n // 16, 1024)               # more slices hold the word than round 2 may take
	for gap in sorted(GAPS):
		gs, gt = GAPS[gap]
		cnt = check(hip, pair, qv, expect_fallback=True, locality=0, gap_s=gs, gap_t=gt, max_matches=10)
		assert cnt[2] > max(pair.n // 16, 1024)


@pytest.mark.parametrize("d", (752, 769))
def test_no_shadow_beside_its_widths(hip, d):
	"""d_pad = 752 and d_pad = 784: VK_BOUND_PASS=force builds no shadow (the same bytes on the device as with `off`), no bound pass
	runs, and the results are the exact pass's"""
	corpus = ragged_with_empties(d, 2000, seed=50 + d)
	with _Env("off"):
		exact = _corpus(hip, corpus["X"], corpus["sent_off"])
	with _Env("force"):
		forced = _corpus(hip, corpus["X"], corpus["sent_off"])
	try:
		assert forced.device_bytes == exact.device_bytes
		for len_t in (10, 16):
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


def test_two_views_from_two_threads(hip):
	p = Pair(hip, synth.make_contextual_corpus(1500, 32, 32, V, 768, seed=61))
	try:
		qs = [q["vectors"] for q in synth.make_queries(p.corpus, 10, 10, seed=77)]
		kw = dict(locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10)
		with _Env("force"):
			alone = [p.forced.query(q, **kw) for q in qs]
			views = [p.forced.view(), p.forced.view()]
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
	finally:
		p.close()
