"""CPU tier of the LP checks of the exact transports ("Exact transports against an LP"): the stored LP scores are current,
the cases are problems in which the exact solver has something to reroute, the oracle agrees with the LP, and the LP helper agrees
with the Hungarian method where the problem is an assignment.  No GPU; the two tests that solve LPs need scipy, the others read the
stored scores."""

import numpy as np
import pytest

import transport_cases as tc
import transport_lp as tl


@pytest.fixture(scope="module")
def golden():
	return tl.load_golden()


@pytest.fixture(scope="module")
def problems(oracle):
	return {c["name"]: tl.Problems(oracle, c) for c in tc.cases()}


def test_shapes_the_cases_must_hold():
	"""the union of the cases holds every query length, slice length and layout the solvers change form at"""
	short_t, short_s, long_s, long_t = set(), set(), set(), set()
	for c in tc.cases():
		lens = set(int(x) for x in np.diff(c["off"]))
		lt = set(len(q["vectors"]) for q in c["queries"])
		if c["search"]:
			assert 700 <= len(c["off"]) - 1 <= 900 and 1 <= min(lens) and max(lens) <= 40
			continue
		if max(lens) > 64:
			assert sum(n > 64 for n in np.diff(c["off"])) <= 8 and any(0 < n <= 64 for n in lens)
			long_s |= {n for n in lens if n > 64}
			long_t |= lt
		short_s |= {n for n in lens if n <= 64}
		short_t |= lt
	assert short_t >= {1, 2, 15, 16, 17, 32, 33, 48, 49, 64}
	assert short_s >= {0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64}
	assert long_s >= {65, 127, 128, 129, 511, 512} and long_t >= {16, 17, 40, 64}
	assert {c["layout"] for c in tc.cases()} == {"contextual", "static"}
	assert {c["family"] for c in tc.cases()} == set(tc.FAMILIES)
	assert sorted(c["family"] for c in tc.cases() if c["search"]) == ["arc", "types"]
	a = tc.case("assignment")
	assert sorted(np.diff(a["off"])) == sorted(len(q["vectors"]) for q in a["queries"]) == [16, 17, 32, 48, 64]


def test_fixture_is_current(oracle, golden):
	"""(a) every case's LP scores, solved again here (all of them, over a pool of processes), are the stored ones within 1e-9, and the
	stored hashes are those of the inputs"""
	pytest.importorskip("scipy")
	fresh = tl.all_scores(oracle)
	for c in tc.cases():
		lp, sha = golden[c["name"]]
		assert sha == tc.input_hash(c) == str(fresh[c["name"] + "/sha256"]), c["name"]
		new = fresh[c["name"] + "/lp"]
		assert lp.shape == new.shape == (len(c["queries"]), len(tc.MODES), len(c["off"]) - 1)
		assert (np.isnan(lp) == np.isnan(new)).all() and (np.isnan(lp) == (np.diff(c["off"]) == 0)[None, None, :]).all()
		np.testing.assert_allclose(new, lp, atol=1e-9, rtol=0, equal_nan=True, err_msg=c["name"])


@pytest.mark.parametrize("family", [f for f in tc.FAMILIES if f != "assignment"])
def test_the_exact_solver_has_something_to_reroute(golden, problems, family):
	"""(b) the LP score is below the nearest-neighbour relaxation's (both directions, oracle.rwmd(injective, symmetric)) by more than
	1e-3 on at least half of the family's non-empty slices -- else every unit of mass sits on its nearest neighbour and the exact
	solver has nothing to do.  Held under both balanced modes, in which the relaxation is one.  Under raw magnitudes and plain bags
	the side in excess is served selectively: the optimum moves only min(sum a, sum b) and lies above the relaxation, which moves all
	of both sides, on most slices of unequal totals (printed, not asserted)."""
	hit, total = {m: 0 for m in tc.MODES}, 0
	for c in tc.cases():
		if c["family"] != family:
			continue
		P = problems[c["name"]]
		lp = golden[c["name"]][0]
		for qi in range(len(c["queries"])):
			rel = np.array([P.relaxed(qi, s) for s in range(P.n_slices())])
			ok = np.isfinite(rel)
			total += int(ok.sum())
			for m in tc.MODES:
				hit[m] += int((lp[qi, tl.mode_index(m)][ok] < rel[ok] - 1e-3).sum())
	print(family, {m: f"{hit[m]}/{total}" for m in tc.MODES})
	for m in ("wrd_norm", "nbow"):
		assert 2 * hit[m] >= total, (family, m, hit[m], total)


def test_skewed_masses_stay_above_the_cutoff(problems):
	"""every mass of the skewed family is at least 1e-6 of its side's total, and the masses do span five orders of magnitude"""
	spread = 0.0
	for c in tc.cases():
		if c["family"] != "skewed":
			continue
		P = problems[c["name"]]
		for s in range(P.n_slices()):
			if P.off[s + 1] - P.off[s] < 1:
				continue
			for qi in range(len(c["queries"])):
				for side in P.masses(qi, s, "wrd_raw"):
					side = side.astype(np.float64)
					assert side.min() >= 1e-6 * side.sum()
					spread = max(spread, side.max() / side.min())
	assert spread >= 1e5


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_oracle_matches_lp(golden, problems, family):
	"""(c) the oracle's raw score of every slice (find over the whole case, nothing pruned) within 1e-6 of the LP"""
	worst = {m: 0.0 for m in tc.MODES}
	for c in tc.cases():
		if c["family"] != family:
			continue
		P = problems[c["name"]]
		lp = golden[c["name"]][0]
		for qi in range(len(c["queries"])):
			for m in tc.MODES:
				raw, _ = P.oracle_scores(qi, m)
				want = lp[qi, tl.mode_index(m)]
				assert (np.isnan(raw) == np.isnan(want)).all()
				ok = np.isfinite(want)
				worst[m] = max(worst[m], float(np.abs(raw[ok] - want[ok]).max()))
	print(family, {m: f"{v:.2e}" for m, v in worst.items()})
	assert max(worst.values()) <= 1e-6, (family, worst)


def test_lp_matches_the_hungarian_method(problems):
	"""(d) len_t == len_s with uniform masses is the assignment problem: the LP's optimum is that of linear_sum_assignment"""
	linear_sum_assignment = pytest.importorskip("scipy.optimize").linear_sum_assignment
	c = tc.case("assignment")
	P = problems["assignment"]
	lens = np.diff(c["off"])
	seen = 0
	for qi, q in enumerate(c["queries"]):
		for s in np.flatnonzero(lens == len(q["vectors"])):
			n = int(lens[s])
			for mode in ("nbow", "bow"):
				a, b, C = P.problem(qi, int(s), mode)
				assert (a == a[0]).all() and (b == a[0]).all()
				r, col = linear_sum_assignment(C)
				assert abs(tl.lp_score(a, b, C) - (1.0 - C[r, col].sum() / n)) <= 1e-9
				seen += 1
	assert seen == 10
