"""-m gpu: the bound pass over the compact 6-bit shadow (VK_BOUND_PASS=force VK_BOUND_BITS=6c: 3,712-byte tiles, MODE 9)
against the exact pass it stands in for, by the claims of tests/test_gpu_bound6_pass.py.  Every case runs one query on two handles
of the same vectors -- one with a compact shadow, one with none (VK_BOUND_PASS=off) -- and asserts
  (a) the bound of every non-empty slice is >= the exact pass's score of it, and -inf for the empty ones;
  (b) the two result sets are the same arrays, byte for byte, and so are last_scores();
  (c) under the caller's own gap table (linear, affine, general with VK_BOUND_TAIL=0) bound - exact <= delta and round 2 holds at
      most round2_limit(delta) slices, delta from the numpy statement of the compact quantizer (tests/bound6c_cases.py: s and e
      rounded up to bf16); under VK_BOUND_TAIL=1 the bound is that of a cheaper table and only (a), (b) and (e) are claimed;
  (d) no fallback wherever that limit is within max(n / 16, 1024), the line tests/test_gpu_bound6_pass.py draws; beyond it either
      outcome is right;
  (e) for one-token queries under local alignment a slice's bound is the largest cell over its tokens (one query column: no gap can
      pay), so the bounds the handle reports (vk_bound_pass_state, as tests/test_gpu_bound_tail.py reads them) equal the numpy
      statement of the cell bit for bit -- clip01(((s_x cs) I + e_x ca) + cb) in float32 in the kernel's order, s_x and e_x the bf16
      values of the compact tile, I the exact product of the codes -- under every gap form, the flat-tailed ones included.
Corpora of 1,500 slices at 300-d: 32 tokens each; 24 tokens each (every second slice straddles two tiles); ragged of 8 .. 32 and of
33 .. 64 tokens (the 64-row history).  Gaps: linear, affine, general (exp5) with VK_BOUND_TAIL 0 and 1; queries of 1, 4, 10, 12 and
16 tokens.  VK_BOUND_BITS=6 on the same vectors still builds 3,968-byte tiles and gives the same results."""

import ctypes as C

import numpy as np
import pytest

import bound6_cases as b6
import bound6c_cases as b6c
import bound_cases as bc
from bound_cases import case_queries, same_results, state
from vectorian_amd import synth

pytestmark = pytest.mark.gpu

F = np.float32
D, V, N = 300, 50_000, 1500
EXP5 = ("table", (1 - 2.0 ** (-np.arange(0, 65) / 5)).astype(F))
GAPS = {"linear": (0.1, 0.1, None), "affine": (("affine", 0.2, 0.05), ("affine", 0.2, 0.05), None), "exp5": (EXP5, EXP5, "0"), "exp5 tail": (EXP5, EXP5, "1")}
SHAPES = {"32": (32, 32, 71), "24": (24, 24, 72), "8..32": (8, 32, 73), "33..64": (33, 64, 74)}


def _Env(mode, tail=None, bits="6c"):
	return bc.Env(VK_BOUND_PASS=mode, VK_BOUND_BITS=bits, VK_BOUND_TAIL=tail)


def _int_of(hip, c, name, ctype):
	"""vk_bound_pass_bits / vk_bound_pass_tail of a handle"""
	fn = getattr(hip.lib(), name)
	fn.restype = C.c_int
	fn.argtypes = [C.c_void_p, C.c_void_p]
	out = ctype(-1)
	with c.lock:
		hip._check(fn(c._h, C.byref(out)))
	return out.value


def bits_of(hip, c):
	return _int_of(hip, c, "vk_bound_pass_bits", C.c_int64)


def tail_of(hip, c):
	return _int_of(hip, c, "vk_bound_pass_tail", C.c_int32)


class Pair(bc.Pair):
	"""the same vectors twice: `forced` has a compact shadow, `exact` has none; the compact quantizer's statement of every row"""

	def __init__(self, hip, corpus):
		super().__init__(hip, lambda mode: _Env(mode), corpus)
		fmt, self.N, self.Xmax, _ = bc.shadow_of(hip, self.forced, 0, 0)
		assert fmt["bits"] == 6 and fmt["tile_bytes"] == b6c.TILE and fmt["live"] == 2 and bits_of(hip, self.forced) == 6
		tiles = self.X.shape[0] // 16
		extra = self.forced.device_bytes - self.exact.device_bytes
		assert tiles * b6c.TILE <= extra <= (tiles + 8) * b6c.TILE + 4096, (extra, tiles)   # the shadow is counted at its real size
		self.codes, self.s, self.e, n, a = b6c.quantize6c(b6.stored(self.X))
		assert self.N.view(np.uint32) == n.max().view(np.uint32) and self.Xmax.view(np.uint32) == a.max().view(np.uint32)
		self.terms = (float(self.e.max()) * (1 + 1e-5), float(n.max()) * (1 + 1e-5), float(a.max()) * (1 + 1e-5))
		self.lens = np.diff(self.off)

	def cells(self, q_stored):
		"""[tokens, len_t] float32: the numpy statement of the bound cell against every token of the corpus"""
		qc, s_q, e_q, _, a_q = b6.quantize6(q_stored)
		cs, ca, cb = b6.constants(s_q, e_q, a_q, self.N, self.Xmax)
		P = ((b6.EIGHTHS[self.codes] @ b6.EIGHTHS[qc].T).astype(np.float64) / 64).astype(F)   # exact: multiples of 1 / 64 below 2^15
		ub = ((self.s[:, None] * cs[None, :]).astype(F) * P).astype(F)
		ub = ((ub + (self.e[:, None] * ca[None, :]).astype(F)).astype(F) + cb[None, :]).astype(F)
		return np.clip(ub, F(0), F(1))


@pytest.fixture(scope="module")
def pairs(hip):
	made = {}

	def get(name):
		if name not in made:
			lo, hi, seed = SHAPES[name]
			made[name] = Pair(hip, synth.make_contextual_corpus(N, lo, hi, V, D, seed=seed))
		return made[name]
	yield get
	for p in made.values():
		p.close()


def check(hip, pair, qv, gap, locality, k=10):
	gs, gt, tail = GAPS[gap]
	kw = dict(locality=locality, gap_s=gs, gap_t=gt, max_matches=k, min_score=0.0 if locality == 0 else -1e9)
	with _Env("force", tail):
		got = pair.forced.query(qv, **kw)
		ub, cnt = state(hip, pair.forced)
		mine = pair.forced.last_scores()
		assert (tail_of(hip, pair.forced) > 0) == (tail == "1")
	with _Env("off", tail):
		ref = pair.exact.query(qv, **kw)
		full = pair.exact.last_scores()
	assert cnt[0] == 1, cnt
	nonempty = pair.lens > 0
	slack = float((ub[nonempty] - full[nonempty]).max())
	print(f"{gap} len_t {len(qv)} locality {locality}: round 1 {cnt[1]}, round 2 {cnt[2]}, fell back {cnt[3]}, bound - exact: max {slack:.5f}")
	assert (ub[nonempty] >= full[nonempty]).all(), (ub[nonempty] - full[nonempty]).min()      # (a)
	assert np.isneginf(ub[~nonempty]).all()
	same_results(got, ref)                                                                    # (b)
	assert (mine.view(np.uint32) == full.view(np.uint32)).all()
	if tail != "1":
		delta = b6.delta6(pair.terms, b6.stored(qv))
		limit = b6.round2_limit(delta, full, k, pair.n, kw["min_score"])
		if limit <= max(pair.n // 16, 1024):
			assert cnt[3] == 0, (cnt, limit)                                                  # (d)
		if cnt[3] == 0:
			print(f"  round 2 {cnt[2]} <= {limit}, delta {delta:.5f}")
			assert slack <= delta, (slack, delta)                                             # (c)
			assert cnt[2] <= limit, (cnt, limit)
	return ub


@pytest.mark.parametrize("gap", sorted(GAPS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pruned_query_is_the_exact_query(hip, pairs, shape, gap):
	pair = pairs(shape)
	for len_t in (1, 4, 10, 12, 16):
		for qv in case_queries(pair.corpus, len_t):
			for locality in (0, 2):
				ub = check(hip, pair, qv, gap, locality)
				if len_t == 1 and locality == 0:
					cell = pair.cells(b6.stored(qv))[:, 0]                                   # (e)
					want = np.array([cell[a:b].max() if b > a else -np.inf for a, b in zip(pair.off[:-1], pair.off[1:])], dtype=F)
					assert (ub.view(np.uint32) == want.view(np.uint32)).all(), np.flatnonzero(ub != want)[:8]


def test_six_without_the_c_keeps_the_wide_tiles(hip, pairs):
	pair = pairs("8..32")
	with _Env("force", bits="6"):
		wide = bc.corpus_of(hip, pair.X, pair.off)
	try:
		fmt, _, _, _ = bc.shadow_of(hip, wide, 0, 0)
		assert fmt["bits"] == 6 and fmt["tile_bytes"] == 3968 and fmt["live"] == 2
		for qv in case_queries(pair.corpus, 10):
			kw = dict(locality=0, gap_s=EXP5, gap_t=EXP5, max_matches=10)
			with _Env("force", bits="6"):
				a = wide.query(qv, **kw)
				assert state(hip, wide, bounds=False)[1][0] == 1
			with _Env("force"):
				b = pair.forced.query(qv, **kw)
			same_results(a, b)
	finally:
		wide.close()
