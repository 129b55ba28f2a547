"""-m gpu: the bound pass on vk_score_local_kernel (vk_score_m9f.hip): under local alignment the flat-tailed bound pass
over the compact 6-bit shadow scores a group of four slices of exactly 32 tokens with the straight-line DP dp_tail_local_full and every
other group with dp_general_tail_reg under a compile-time locality and column count.  Both are bit-identical to the form
vk_score_kernel<9, 3, false, 8, LT> calls, which VK_BOUND_DP=generic keeps -- so every case runs one query twice on a handle with the
shadow (VK_BOUND_PASS=force VK_BOUND_BITS=6c VK_BOUND_TAIL=1), with the switch and without it, and once on a handle without a shadow,
and asserts
  (a) the two bound arrays (vk_bound_pass_state) are the same uint32 patterns;
  (b) vk_bound_pass_dp says 1 for a local query without the switch, and 0 with the switch or under global / semiglobal locality;
  (c) the result set of either run is the exact handle's (same_results);
  (d) bound >= exact score for every non-empty slice (-inf for the empty ones).
Corpora at 300-d, 403 slices each:
  full   32 tokens each: a hundred full groups and a last group with an empty slot;
  mixed  32 tokens each, every seventh slice replaced by one of 0, 1, K, K + 1 or 31 tokens (K the compiled tail length): full and
         ragged groups next to each other inside a wave's run of four groups;
  short  16 tokens each: the straight-line form is never taken.
Queries of 1, 2, 4, 5, 8, 9, 10, 12, 13 and 16 tokens (every strip width LT = 4, 8, 12, 16 at both ends), one planted and one drawn;
the slice-gap tables of tests/test_gpu_bound_tail.py (exp5, a constant, one that dips, one that rises steeply); local, global and
semiglobal alignment."""

import ctypes as C

import numpy as np
import pytest

import bound_cases as bc
from bound_cases import same_results, state
from vectorian_amd import synth

pytestmark = pytest.mark.gpu

F = np.float32
D, V, N = 300, 50_000, 403
KS = np.arange(0, 65)
TABLES = {
	"exp5": (1 - 2.0 ** (-KS / 5)).astype(F),
	"constant": np.where(KS > 0, 0.3, 0.0).astype(F),
	# rises, then dips twice: the minimum over K < k <= 32 lies at 20 for every K < 19
	"dips": np.where(KS == 20, 0.12, np.where(KS == 40, 0.07, 0.15 + 0.02 * np.minimum(KS, 12) + 0.05 * np.cos(KS))).astype(F) * (KS > 0),
	"steep": (0.15 * KS).astype(F),
}
EXP5 = ("table", TABLES["exp5"])
LENGTHS = (1, 2, 4, 5, 8, 9, 10, 12, 13, 16)
CORPORA = ("full", "mixed", "short")
COMPACT_TILE = 3712


def _Env(mode, dp=None):
	return bc.Env(VK_BOUND_PASS=mode, VK_BOUND_BITS="6c", VK_BOUND_TAIL="1", VK_BOUND_DP=dp)


def _int_of(hip, c, name):
	fn = getattr(hip.lib(), name)
	fn.restype = C.c_int
	fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
	out = C.c_int32(-1)
	with c.lock:
		hip._check(fn(c._h, C.byref(out)))
	return out.value


def dp_of(hip, c):
	"""vk_bound_pass_dp: 1 where the last bound pass ran vk_score_local_kernel, else 0"""
	return _int_of(hip, c, "vk_bound_pass_dp")


def compiled_k(hip):
	fn = hip.lib().vk_score_m8t_tail_k
	fn.restype = C.c_int32
	fn.argtypes = []
	return int(fn())


def lengths_of(name, k):
	lens = np.full(N, 16 if name == "short" else 32, dtype=np.int64)
	if name == "mixed":
		odd = (0, 1, k, k + 1, 31)
		at = np.arange(3, N, 7)
		lens[at] = [odd[i % len(odd)] for i in range(len(at))]
		groups = lens[:N // 4 * 4].reshape(-1, 4)
		full = (groups == 32).all(axis=1)
		assert full.any() and (~full).any() and (full[:-1] != full[1:]).any() and set(odd) <= set(lens.tolist())
	return lens


def corpus_of(name, k, seed):
	"""the vectors of a 32-token corpus cut into the slices of `name`"""
	corpus = synth.make_contextual_corpus(N, 32, 32, V, D, seed=seed)
	off = np.concatenate([[0], np.cumsum(lengths_of(name, k))]).astype(np.int64)
	corpus["sent_off"] = off
	corpus["X"] = np.ascontiguousarray(corpus["X"][:off[-1]])
	corpus["tok_id"] = corpus["tok_id"][:off[-1]]
	return corpus


@pytest.fixture(scope="module")
def pairs(hip):
	made = {}
	k = compiled_k(hip)
	assert 1 <= k < 30

	def get(name):
		if name not in made:
			pair = bc.Pair(hip, lambda mode: _Env(mode), corpus_of(name, k, 81 + CORPORA.index(name)))
			fmt, _, _, _ = bc.shadow_of(hip, pair.forced, 0, 0)
			assert fmt["bits"] == 6 and fmt["tile_bytes"] == COMPACT_TILE, fmt   # the compact shadow: MODE 9
			assert pair.n == N and N % 4 == 3                                       # the last group has an empty slot
			made[name] = pair
		return made[name]
	yield get
	for p in made.values():
		p.close()


def check(hip, pair, w, qv, locality):
	kw = dict(locality=locality, gap_s=("table", w), gap_t=EXP5, want_flow=False, max_matches=10, min_score=0.0 if locality == 0 else -1e9)
	with _Env("force"):
		got = pair.forced.query(qv, **kw)
		ub, cnt = state(hip, pair.forced)
		ran = dp_of(hip, pair.forced)
	with _Env("force", "generic"):
		got_generic = pair.forced.query(qv, **kw)
		ub_generic, cnt_generic = state(hip, pair.forced)
		ran_generic = dp_of(hip, pair.forced)
	with _Env("off"):
		ref = pair.exact.query(qv, **kw)
		full = pair.exact.last_scores()
		assert dp_of(hip, pair.exact) == 0
	assert cnt[0] == 1 and cnt_generic[0] == 1
	differ = int((ub.view(np.uint32) != ub_generic.view(np.uint32)).sum())
	print(f"len_t {len(qv)} locality {locality}: kernel {ran} / {ran_generic}, bounds that differ {differ}, round 2 {cnt[2]} / {cnt_generic[2]}")
	assert differ == 0, differ                                                             # (a)
	assert ran == (1 if locality == 0 else 0) and ran_generic == 0, (ran, ran_generic)     # (b)
	same_results(got, ref)                                                                 # (c)
	same_results(got_generic, ref)
	nonempty = np.diff(pair.off) > 0
	assert (ub[nonempty] >= full[nonempty]).all(), (ub[nonempty] - full[nonempty]).min()   # (d)
	assert np.isneginf(ub[~nonempty]).all()


def test_the_corpora_are_what_the_module_says():
	for k in (3, 4, 6):
		assert (lengths_of("full", k) == 32).all() and (lengths_of("short", k) == 16).all()
		mixed = lengths_of("mixed", k)
		assert (mixed != 32).sum() == len(range(3, N, 7)) and (mixed[np.arange(N) % 7 != 3] == 32).all()
		assert int(np.argmin(TABLES["dips"][k + 1:33])) + k + 1 == 20
	assert (TABLES["dips"][1:] > 0).all() and (np.diff(TABLES["dips"]) < 0).any()


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("name", CORPORA)
def test_fast_dp_bounds_are_the_generic_bounds(hip, pairs, name, table):
	pair = pairs(name)
	for len_t in LENGTHS:
		for q in synth.make_queries(pair.corpus, 2, len_t, seed=100 + len_t):
			for locality in (0, 1, 2):
				check(hip, pair, TABLES[table], q["vectors"], locality)
