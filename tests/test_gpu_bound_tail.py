"""-m gpu: the bound pass under a slice-gap table that is flat beyond K entries (GAP 8 / 9 of vk_score_kernel).
With VK_BOUND_TAIL=1 a query with general gaps has its bounds computed under
    w'(k) = w(k) for k <= K,   w'(k) = c_tail = min over K < j <= rows of w(j) for k > K     (rows: 32, or 64 where a slice is longer)
by dp_general_tail_reg, which is bit-identical to the present general form fed w' -- so every case runs one query three ways,
  tail:   VK_BOUND_PASS=force VK_BOUND_TAIL=1, the caller's table w;
  plain:  VK_BOUND_PASS=force VK_BOUND_TAIL=0, gap_s = w' built here;
  exact:  VK_BOUND_PASS=off on a handle without a shadow, the caller's table w,
and asserts
  (a) the bounds of `tail` equal those of `plain` bit for bit; vk_bound_pass_tail says K after `tail` and 0 after `plain`;
  (b) the result set of `tail` is that of `exact` (same_results);
  (c) bound >= exact score for every non-empty slice;
  (d) the reported size of round 2 is the count recomputed on the host from the bounds and the exact scores as vk_query.cpp takes its
      rounds (and tools/sim_bound_bits.py restates them): the M = 64 largest bounds above the floor, theta = the kk-th best exact score
      among them (the floor where fewer are above it), then bound >= theta.  Where bounds tie across the 64th place the library may
      take any of the tied slices: the counts under the choice with the lowest and with the highest theta bracket the reported one;
  (e) the query fell back to the full pass exactly where that count exceeds max(n / 16, 1024) (where the bracket straddles the line,
      either).
The queries ask for no traceback, so that kk = max_matches and the floor is min_score itself.
Corpora of 2,000 slices at 300-d (6-bit and 8-bit shadows) and 1,000 at 768-d: lengths 0 .. 32 (the 32-row form) and 0 .. 64 (the
64-row form), every length present, K, K + 1, K + 2, 31 / 32 and 33 / 63 / 64 among them.  Tables: exp5, a constant, one that is not
monotone and has its tail's minimum beyond K + 1, one that rises steeply (a tail that matters).  Linear and affine gaps ignore the
switch; force without the variable runs no tail."""

import ctypes as C

import numpy as np
import pytest

import bound_cases as bc
from bound_cases import case_queries, same_results, state
from vectorian_amd import synth

pytestmark = pytest.mark.gpu

F = np.float32
V, M = 50_000, 64
KS = np.arange(0, 65)
TABLES = {
	"exp5": (1 - 2.0 ** (-KS / 5)).astype(F),
	"constant": np.where(KS > 0, 0.3, 0.0).astype(F),
	# rises, then dips twice: the minimum over k > K lies at 40 (64-row forms) and at 20 (32-row forms) for every K < 19
	"dips": np.where(KS == 20, 0.12, np.where(KS == 40, 0.07, 0.15 + 0.02 * np.minimum(KS, 12) + 0.05 * np.cos(KS))).astype(F) * (KS > 0),
	"steep": (0.15 * KS).astype(F),
}
EXP5 = ("table", TABLES["exp5"])


def _Env(mode, bits=None, tail=None):
	return bc.Env(VK_BOUND_PASS=mode, VK_BOUND_BITS=bits, VK_BOUND_TAIL=tail)


def tail_of(hip, c):
	"""vk_bound_pass_tail: K where the last bound pass ran a flat-tailed form, else 0"""
	fn = hip.lib().vk_bound_pass_tail
	fn.restype = C.c_int
	fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
	out = C.c_int32(-1)
	with c.lock:
		hip._check(fn(c._h, C.byref(out)))
	return out.value


def compiled_k(hip, bits):
	fn = getattr(hip.lib(), "vk_score_m8t_tail_k" if bits == 6 else "vk_score_m7t_tail_k")
	fn.restype = C.c_int32
	fn.argtypes = []
	return int(fn())


def flat_tailed(w, k, rows):
	"""w' of the module's text (vk_host::bound_tail_cost restated)"""
	out = w.copy()
	out[k + 1:] = w[k + 1:rows + 1].min()
	return out


def ragged(d, n, longest, seed):
	"""n slices of 0 .. longest tokens: every length 1 .. longest drawn, five slices emptied (first, inside a group, last)"""
	corpus = synth.make_contextual_corpus(n - 5, 1, longest, V, d, seed=seed)
	off = corpus["sent_off"]
	at = np.array([0, 7, (n - 5) // 2, n - 6, n - 5])
	corpus["sent_off"] = np.insert(off, at, off[at])
	assert set(np.diff(corpus["sent_off"]).tolist()) == set(range(0, longest + 1))
	return corpus


class Pair(bc.Pair):
	def __init__(self, hip, corpus, bits):
		self.bits = bits
		super().__init__(hip, lambda mode: _Env(mode, bits=str(bits)), corpus)
		self.rows = 32 if int(np.diff(self.off).max()) <= 32 else 64
		self.k = compiled_k(hip, bits)
		assert 1 <= self.k < 31


def _pair(hip, d, n, longest, bits, seed):
	p = Pair(hip, ragged(d, n, longest, seed), bits)
	return p


@pytest.fixture(scope="module")
def pairs(hip):
	made = {}

	def get(name):
		if name not in made:
			d, n, longest, bits, seed = {"6/32": (300, 2000, 32, 6, 61), "6/64": (300, 2000, 64, 6, 62), "8/32": (300, 2000, 32, 8, 63),
				"8/64": (300, 2000, 64, 8, 64), "768/32": (768, 1000, 32, 8, 65), "768/64": (768, 1000, 64, 8, 66)}[name]
			made[name] = _pair(hip, d, n, longest, bits, seed)
		return made[name]
	yield get
	for p in made.values():
		p.close()


def round2_bracket(ub, full, kk, floor):
	"""(fewest, most) slices of round 2 over the admissible choices of round 1 (claim (d))"""
	cand = np.nonzero(ub > floor)[0]
	if len(cand) == 0:
		return 0, 0
	order = cand[np.argsort(-ub[cand], kind="stable")]
	sure, tied, need = order[:M], np.empty(0, dtype=np.int64), 0
	if len(order) > M and ub[order[M - 1]] == ub[order[M]]:
		edge = ub[order[M - 1]]
		sure = order[ub[order] > edge]
		tied = order[ub[order] == edge]
		need = M - len(sure)

	def count(first):
		best = np.sort(full[first][full[first] > floor])[::-1]
		theta = best[kk - 1] if len(best) >= kk else floor
		return int(((ub >= theta) & (ub > floor)).sum())
	if need == 0:
		c = count(sure)
		return c, c
	by_exact = tied[np.argsort(full[tied], kind="stable")]
	low_theta, high_theta = count(np.concatenate([sure, by_exact[:need]])), count(np.concatenate([sure, by_exact[-need:]]))
	return min(low_theta, high_theta), max(low_theta, high_theta)


def check(hip, pair, w, qv, **kw):
	"""one query the three ways of the module's text: (a) .. (e); returns (the counters of `tail`, max bound(w') - bound-free exact)"""
	kw = dict(kw, want_flow=False, gap_t=EXP5)
	wp = flat_tailed(w, pair.k, pair.rows)
	bits = str(pair.bits)
	with _Env("force", bits, "1"):
		got = pair.forced.query(qv, gap_s=("table", w), **kw)
		ub, cnt = state(hip, pair.forced)
		assert tail_of(hip, pair.forced) == pair.k
	with _Env("force", bits, "0"):
		pair.forced.query(qv, gap_s=("table", wp), **kw)
		ub_plain, cnt_plain = state(hip, pair.forced)
		assert tail_of(hip, pair.forced) == 0
	with _Env("off", bits):
		ref = pair.exact.query(qv, gap_s=("table", w), **kw)
		full = pair.exact.last_scores()
		assert tail_of(hip, pair.exact) == 0
	assert cnt[0] == 1 and cnt_plain[0] == 1
	assert (ub.view(np.uint32) == ub_plain.view(np.uint32)).all(), np.abs(ub - ub_plain).max()          # (a)
	same_results(got, ref)                                                                               # (b)
	nonempty = np.diff(pair.off) > 0
	assert (ub[nonempty] >= full[nonempty]).all(), (ub[nonempty] - full[nonempty]).min()                 # (c)
	assert np.isneginf(ub[~nonempty]).all()
	lo, hi = round2_bracket(ub, full, kw["max_matches"], F(kw.get("min_score", 0.0)))
	line = max(pair.n // 16, 1024)
	print(f"bits {pair.bits} rows {pair.rows} len_t {len(qv)} locality {kw.get('locality')}: round 2 {cnt[2]} in [{lo}, {hi}], fell back {cnt[3]}")
	assert cnt[1] == M and lo <= cnt[2] <= hi, (cnt, lo, hi)                                             # (d)
	if lo > line:
		assert cnt[3] == 1, (cnt, lo)                                                                    # (e)
	elif hi <= line:
		assert cnt[3] == 0, (cnt, hi)
	assert cnt[3] == int(cnt[2] > line)
	return cnt


def sweep(hip, pair, table):
	w = TABLES[table]
	for len_t in (1, 4, 10, 16):
		for qv in case_queries(pair.corpus, len_t):
			for locality in (0, 1, 2):
				check(hip, pair, w, qv, locality=locality, max_matches=10, min_score=0.0 if locality == 0 else -1e9)


def test_the_tables_are_what_the_module_says():
	for k in (3, 4, 6):
		assert int(np.argmin(TABLES["dips"][k + 1:33])) + k + 1 == 20 and int(np.argmin(TABLES["dips"][k + 1:65])) + k + 1 == 40
		assert (TABLES["dips"][1:] > 0).all() and (np.diff(TABLES["dips"]) < 0).any()
		assert flat_tailed(TABLES["steep"], k, 32)[32] == TABLES["steep"][k + 1] < TABLES["steep"][32]
		assert (flat_tailed(TABLES["constant"], k, 64) == TABLES["constant"]).all()


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("shape", ("6/32", "6/64", "8/32", "8/64"))
def test_tail_bounds_are_the_general_forms_under_the_flat_table(hip, pairs, shape, table):
	sweep(hip, pairs(shape), table)


@pytest.mark.parametrize("shape", ("768/32", "768/64"))
def test_tail_at_768_features(hip, pairs, shape):
	pair = pairs(shape)
	for table in ("exp5", "steep"):
		w = TABLES[table]
		for len_t in (4, 10):
			for qv in case_queries(pair.corpus, len_t):
				for locality in (0, 1, 2):
					check(hip, pair, w, qv, locality=locality, max_matches=10, min_score=0.0 if locality == 0 else -1e9)


@pytest.mark.parametrize("shape", ("6/64", "8/64"))
def test_a_frequent_word_falls_back_under_the_tail_too(hip, pairs, shape):
	"""claim (e) on its other side: a one-token query for the corpus's most frequent word (a twentieth of all tokens: four slices in
	five of 1 .. 64 tokens hold it and tie within the quantization error) has more than max(n / 16, 1024) slices in round 2"""
	pair = pairs(shape)
	rng = np.random.default_rng(2)
	qv = (pair.corpus["E"][0] + 0.05 * rng.standard_normal(pair.X.shape[1])).astype(F)[None, :]
	assert (pair.corpus["tok_id"] == 0).mean() > 0.05
	for table in ("exp5", "steep"):
		cnt = check(hip, pair, TABLES[table], qv, locality=0, max_matches=10)
		assert cnt[3] == 1 and cnt[2] > max(pair.n // 16, 1024), cnt


@pytest.mark.parametrize("shape", ("6/32", "8/64"))
def test_linear_and_affine_gaps_ignore_the_switch(hip, pairs, shape):
	pair = pairs(shape)
	bits = str(pair.bits)
	for gs, gt in ((0.1, 0.1), (("affine", 0.2, 0.05), ("affine", 0.2, 0.05))):
		for qv in case_queries(pair.corpus, 10):
			kw = dict(locality=0, gap_s=gs, gap_t=gt, max_matches=10)
			with _Env("force", bits, "1"):
				got = pair.forced.query(qv, **kw)
				ub, cnt = state(hip, pair.forced)
				assert cnt[0] == 1 and tail_of(hip, pair.forced) == 0
			with _Env("force", bits, "0"):
				same_results(pair.forced.query(qv, **kw), got)
				ub0, cnt0 = state(hip, pair.forced)
			assert (ub.view(np.uint32) == ub0.view(np.uint32)).all() and (cnt[:4] == cnt0[:4]).all()


@pytest.mark.parametrize("shape", ("6/32", "8/64"))
def test_force_without_the_variable_runs_no_tail(hip, pairs, shape):
	pair = pairs(shape)
	bits = str(pair.bits)
	qv = case_queries(pair.corpus, 10)[0]
	kw = dict(locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10)
	with _Env("force", bits, None):
		got = pair.forced.query(qv, **kw)
		ub, cnt = state(hip, pair.forced)
		assert cnt[0] == 1 and tail_of(hip, pair.forced) == 0
	with _Env("force", bits, "0"):
		same_results(pair.forced.query(qv, **kw), got)
		assert (state(hip, pair.forced)[0].view(np.uint32) == ub.view(np.uint32)).all()
	with _Env("force", bits, "1"):
		same_results(pair.forced.query(qv, **kw), got)
		assert tail_of(hip, pair.forced) == pair.k
