"""-m gpu: the exact stage of WRD and full WMD (vk_wrd_exact_kernel<1..4>, vk_wrd_exact_long_kernel<1|4>) against an independent
float64 LP on degenerate problems (transport_cases.py; DESIGN 7, "Exact transports against an LP"): every slice of every case, not
only winners (only_slices: no bound pass, nothing pruned), every plan held to be optimal, and the search route over corpora of more
slices than round 1 takes.  The LP scores come from tests/golden/transport_lp.npz (test_transport_lp_host.py keeps it current);
nothing here imports scipy.

The tolerance on raw_score, 2e-6, is derived: the score is (float)(num / den), num a double sum of float products (1 - c) (float)g
-- two float roundings per term, at most 1.2e-7 den in all --, one float cast adds 6e-8, mass left below EPS at most (n + m) 1e-13,
the LP at 1e-9 tolerances well under 1e-7: about 2.4e-7, and 2e-6 leaves a factor of eight."""

import time

import numpy as np
import pytest

import transport_cases as tc
import transport_lp as tl
from helpers import assert_same_results

pytestmark = pytest.mark.gpu

RAW_TOL = 2e-6
MASS_TOL = 1e-6
F32 = 2.0 ** -24   # relative rounding of a float32
CHUNK = 512   # listed slices per call (at most 1,024): the 800-slice corpora take two calls


@pytest.fixture(scope="module")
def golden():
	return tl.load_golden()


def make_corpus(hip, c):
	n_tokens, n = int(c["off"][-1]), len(c["off"]) - 1
	if c["layout"] == "static":
		h = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=c["d"], n_tokens=n_tokens, n_sentences=n, vocab_size=len(c["E"]), keep_magnitudes=True)
		h.append_vectors(c["E"], normalize=True)
		h.set_token_ids(c["tok_id"])
	else:
		h = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=c["d"], n_tokens=n_tokens, n_sentences=n, keep_magnitudes=True)
		h.append_vectors(c["X"], normalize=True)
	h.set_sentences(c["off"])
	h.finalize()
	return h


def run(hip, h, c, qi, mode, **kw):
	alg, opts = tc.MODES[mode]
	q = c["queries"][qi]
	if "ids" in q:
		kw["q_token_ids"] = q["ids"]
	return h.query(q["vectors"], algorithm=hip.VK_ALG_WRD if alg == "wrd" else hip.VK_ALG_RWMD, q_normalize=True, **opts, **kw)


def check_plan(P, qi, s, mode, plan, lp):
	"""the plan of one slice, evaluated in float64: feasible, moves all it can, and optimal (its value is the LP's); returns its
	distance to the LP score"""
	a, b, C = P.problem(qi, s, mode)
	n, m = C.shape
	assert (plan >= 0).all()
	assert not plan[n:].any() and not plan[:, m:].any()
	G = plan[:n, :m].astype(np.float64)
	rows, cols, moved = G.sum(axis=1), G.sum(axis=0), min(a.sum(), b.sum())
	# the plan is stated in float32: every entry is rounded by at most 2^-24 of itself, a row or column by at most 2^-24 of its mass
	# (6e-8 for normalised masses; raw magnitudes reach 1e4, where an ulp alone is 1e-3)
	ra, rb, rt = MASS_TOL + F32 * a, MASS_TOL + F32 * b, MASS_TOL + F32 * moved
	assert (rows <= a + ra).all(), (s, mode, float((rows - a).max()))
	assert (cols <= b + rb).all(), (s, mode, float((cols - b).max()))
	assert abs(G.sum() - moved) <= rt, (s, mode, G.sum(), moved)
	if mode in ("wrd_norm", "nbow"):
		# balanced up to the rounding of the masses (a 511-token slice's float32 sum of magnitudes is off by 1e-6 of itself, so are
		# its masses' total): the side of the smaller total is used up, the other side is short of its masses by the difference in all
		small, large = ((rows, a, ra), (cols, b, rb)) if a.sum() <= b.sum() else ((cols, b, rb), (rows, a, ra))
		assert (np.abs(small[0] - small[1]) <= small[2]).all(), (s, mode)
		assert abs((large[1] - large[0]).sum() - abs(a.sum() - b.sum())) <= rt, (s, mode)
	value = 1.0 - (C * G).sum() / G.sum()
	assert abs(value - lp) <= RAW_TOL, (s, mode, value, lp)
	return abs(value - lp)


# a case runs its four modes in one test, or (per_mode: one long slice that takes the long solver seconds) each in a test of its own
EVERY_SLICE = [(c["name"], m) for c in tc.cases() for m in (list(tc.MODES) if c["per_mode"] else [None])]


@pytest.mark.parametrize("name,only_mode", EVERY_SLICE, ids=[n if m is None else f"{n}-{m}" for n, m in EVERY_SLICE])
def test_every_slice_against_the_lp(hip, oracle, golden, name, only_mode):
	"""every slice of the case listed in a shuffled order, under every query and mode: raw_score within 2e-6 of the LP, score within
	the project's 1e-5 (2e-5 beyond 16 query tokens) of the oracle's, -inf for an empty slice, and the plan optimal"""
	c = tc.case(name)
	modes = list(tc.MODES) if only_mode is None else [only_mode]
	lp_all, sha = golden[name]
	assert sha == tc.input_hash(c)
	P = tl.Problems(oracle, c)
	h = make_corpus(hip, c)
	n = P.n_slices()
	rng = np.random.default_rng(7)
	worst = {m: 0.0 for m in modes}
	worst_plan = {m: 0.0 for m in modes}
	t_gpu, calls = 0.0, []
	for qi, q in enumerate(c["queries"]):
		len_t = len(q["vectors"])
		for mode in modes:
			lp = lp_all[qi, tl.mode_index(mode)]
			_, ref_score = P.oracle_scores(qi, mode)
			order = rng.permutation(n).astype(np.int64)
			for k in range(0, n, CHUNK):
				ids = order[k:k + CHUNK]
				t0 = time.perf_counter()
				got = run(hip, h, c, qi, mode, only_slices=ids)
				t_gpu += time.perf_counter() - t0
				calls.append((round(time.perf_counter() - t0, 2), len_t, mode))
				assert got.n == len(ids) and (got.sentence[:got.n] == ids).all()
				raw, score = got.raw_score[:got.n].astype(np.float64), got.score[:got.n].astype(np.float64)
				empty = np.isnan(lp[ids])
				assert (raw[empty] == -np.inf).all() and (score[empty] == -np.inf).all()
				err = np.abs(raw[~empty] - lp[ids][~empty])
				worst[mode] = max(worst[mode], float(err.max()))
				assert (err <= RAW_TOL).all(), (name, qi, mode, ids[~empty][np.argmax(err)], float(err.max()))
				assert (np.abs(score[~empty] - ref_score[ids][~empty]) <= (1e-5 if len_t <= 16 else 2e-5)).all(), (name, qi, mode)
				assert got.plan is not None
				for i in np.flatnonzero(~empty):
					worst_plan[mode] = max(worst_plan[mode], check_plan(P, qi, int(ids[i]), mode, got.plan[i], lp[ids[i]]))
	h.close()
	print(f"\n{name}: worst |raw_score - LP| {({m: f'{v:.2e}' for m, v in worst.items()})}, "
		f"worst |plan's value - LP| {({m: f'{v:.2e}' for m, v in worst_plan.items()})}, {t_gpu:.2f} s in query(), the slowest calls (s, len_t, mode) {sorted(calls)[-3:]}")


@pytest.mark.parametrize("mode", list(tc.MODES))
@pytest.mark.parametrize("name", [c["name"] for c in tc.cases() if c["search"]])
def test_search_route_against_the_lp(hip, oracle, golden, name, mode, monkeypatch, capfd):
	"""the bound pass and both candidate rounds: the result set is the LP's -- a slice the bound prunes wrongly under ties shows as a
	missing winner.  The library's score is the raw score over the query length (vko_score), so the reference is stated from the LP
	scores through that formula, and raw_score is held against the LP itself.  Whether round 2 ran is read from the library's own
	report (VK_DEBUG_CANDIDATES): under the balanced modes it must have, for some query of the corpus."""
	c = tc.case(name)
	lp_all, sha = golden[name]
	assert sha == tc.input_hash(c)
	P = tl.Problems(oracle, c)
	h = make_corpus(hip, c)
	monkeypatch.setenv("VK_DEBUG_CANDIDATES", "1")
	capfd.readouterr()
	round2 = []
	for qi, q in enumerate(c["queries"]):
		lp = lp_all[qi, tl.mode_index(mode)]
		len_t = len(q["vectors"])
		score = np.array([oracle.score(np.float32(x), len_t, len_t) for x in lp], dtype=np.float32)
		by_rank = np.lexsort((-np.arange(len(lp)), -score.astype(np.float64)))   # score descending, then slice index descending
		for max_matches in (1, 10, 64):
			for min_score in (0.0, -10.0):
				keep = [int(s) for s in by_rank if score[s] > min_score][:max_matches]
				ref = dict(score=score[keep], sentence=np.array(keep, dtype=np.int64))
				for want_flow in (True, False):
					got = run(hip, h, c, qi, mode, max_matches=max_matches, min_score=min_score, want_flow=want_flow)
					if "round 2 solves" in capfd.readouterr().err:
						round2.append((qi, max_matches, min_score, want_flow))
					assert_same_results(got.trimmed(), ref, check_mapping=False, score_tol=2e-6, tie_tol=2e-6)
					for i in range(got.n):
						s = int(got.sentence[i])
						assert abs(float(got.raw_score[i]) - lp[s]) <= RAW_TOL, (s, got.raw_score[i], lp[s])
						if want_flow:
							check_plan(P, qi, s, mode, got.plan[i], lp[s])
	h.close()
	print(f"\n{name} {mode}: round 2 ran in {len(round2)} of {12 * len(c['queries'])} queries: (query, max_matches) {sorted({(r[0], r[1]) for r in round2})}")
	if mode in ("wrd_norm", "nbow"):
		assert round2, (name, mode)
