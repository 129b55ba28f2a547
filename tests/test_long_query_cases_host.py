"""CPU tier, the oracle alone: the inputs of tests/test_gpu_long_query_gaps_and_ties.py are what that module takes them for, so that it
cannot pass vacuously.  The planted phrase makes the maximum of a slice attained twice and the oracle start at the first; the shared
filler makes winners of repeated words, and swapping w_s and w_t moves them; every table has the tail the host's rule gives it, below
the query's length; and on the float corpora a tail moved by one entry, or swapped tables, move the scores by more than twice the
tolerance of the GPU comparison."""

import numpy as np
import pytest

import long_query_cases as L

LOCALITIES = {L.LOCAL: "local", L.GLOBAL: "global", L.SEMIGLOBAL: "semiglobal"}


def slice_ids(c, s):
	return c["ids"][c["sent_off"][s]:c["sent_off"][s + 1]]


def test_the_corpora_are_what_they_say():
	for stream in L.STREAMS:
		c = L.corpus_of(stream)
		lens = c["lens"]
		longest = 64 if stream.endswith("64") else 512
		assert {n for n in L.EDGE_LENS if n <= longest} <= set(int(x) for x in lens) and ((lens >= 1) & (lens <= 64)).sum() >= 40 and lens.max() == longest
		assert int(c["sent_off"][-1]) == len(c["ids"]) and c["ids"].max() < L.V
		for name, (n, p1, p2) in (L.SHORT_TRIPLES if longest == 64 else L.TRIPLES).items():
			both, first, second = (slice_ids(c, s) for s in c["triples"][name])
			assert len(both) == len(first) == len(second) == n
			assert (both[p1:p1 + 12] == L.PHRASE).all() and (both[p2:p2 + 12] == L.PHRASE).all() and p2 >= p1 + 12
			assert (first[p1:p1 + 12] == L.PHRASE).all() and (second[p2:p2 + 12] == L.PHRASE).all()
			# otherwise identical, and filler only
			for a in (first, second):
				assert (a != both).sum() == 12 and np.isin(a[a != both], np.arange(*L.SLICE_FILLER)).all()
		# blocks of 64 slice tokens: 0 and 2; one block's lanes (the end cells 16 and 66: blocks 0 and 1); adjacent blocks
		assert (10 + 11) // 64 == 0 and 140 // 64 == 2 and (52 + 11) == 63 and 64 // 64 == 1
	for len_t in L.EXACT_LENS + (160,):
		q = L.exact_query("planted", len_t)
		assert (q[30:42] == L.PHRASE).all() and np.isin(np.delete(q, np.arange(30, 42)), np.arange(*L.QUERY_FILLER)).all()
		assert (L.exact_query("planted", len_t, "end")[-12:] == L.PHRASE).all()
		assert np.isin(L.exact_query("shared", len_t), np.arange(*L.SLICE_FILLER)).all()
	# all costs dyadic: multiples of 1/8 (the concave tables: of 1/64), a gap of 512 tokens at most 1,024 -- every value of the DP is such
	# a multiple within +-2^12 (512 matches, a border and a gap): 18 bits, exact in fp32 in whatever order it is summed
	for s in L.gap_settings(129).values():
		for gap in (s.gap_s, s.gap_t):
			w = np.array([L.cost(gap, k) for k in range(L.N_TABLE)], dtype=np.float64)
			unit = 64 if s.name in L.CONCAVE_SETTINGS else 8
			assert (w * unit == np.round(w * unit)).all() and (w >= 0).all() and w.max() <= 1024, s.name


@pytest.mark.parametrize("len_t", L.EXACT_LENS)
def test_planted_ties(oracle, len_t):
	"""the three slices of a triple score alike to the bit -- the maximum of "both" is attained twice --, and the oracle starts "both"
	where it starts "first only": a kernel that let the later lane or the later block win a tie returns the other mapping"""
	triples = [(c, t, members) for c in (L.corpus_of("planted"), L.corpus_of("planted64")) for t, members in c["triples"].items()]
	for name, loc in L.PLANTED_TIES:
		s = L.gap_settings(len_t)[name]
		q = L.exact_query("planted", len_t, L.query_place("planted", loc))
		for c, triple, members in triples:
			(r_both, m_both), (r_first, m_first), (r_second, m_second) = (oracle.align(L.sim01(slice_ids(c, i), q), loc, s.gap_s, s.gap_t) for i in members)
			where = (name, LOCALITIES[loc], triple)
			assert np.float32(r_both).view(np.uint32) == np.float32(r_first).view(np.uint32) == np.float32(r_second).view(np.uint32), where
			assert r_both == 12.0, where
			assert (m_both == m_first).all(), where
			assert not (m_both == m_second).all(), where
			assert (m_both >= 0).sum() >= 12, where


def test_planted_ties_end_under_global(oracle):
	"""why PLANTED_TIES leaves GLOBAL out: the whole slice is aligned, so the three slices differ"""
	c = L.corpus_of("planted")
	s = L.gap_settings(80)["lin_asym"]
	q = L.exact_query("planted", 80)
	(r0, m0), (r1, m1), (r2, m2) = (oracle.align(L.sim01(slice_ids(c, i), q), L.GLOBAL, s.gap_s, s.gap_t) for i in c["triples"]["t200"])
	assert not (r0 == r1 == r2 and (m0 == m1).all() and not (m0 == m2).all())


def test_the_layouts_share_one_reference(oracle):
	"""0 / 1 similarities: the static layout, the contextual one at d = 64 and d = 300 and fp32 rows give the oracle one answer, which
	the GPU module computes once"""
	for name, loc, len_t, stream in (("lin_asym", L.LOCAL, 65, "shared"), ("aff0", L.GLOBAL, 80, "planted"), ("sat9", L.SEMIGLOBAL, 65, "shared")):
		ref = L.oracle_exact(oracle, stream, name, loc, len_t)
		for kw in (dict(layout="static"), dict(d=300), dict(f32=True), dict(layout="static", d=300)):
			other = L.oracle_exact(oracle, stream, name, loc, len_t, **kw)
			for field in ("score", "raw", "sentence", "mapping", "all_scores"):
				assert (np.asarray(ref[field]) == np.asarray(other[field])).all(), (name, kw, field)


@pytest.mark.parametrize("name", L.SETTINGS)
def test_shared_ties(oracle, name):
	"""the runs over the shared filler: winners of repeated words (co-optimal tracebacks), and w_s / w_t swapped move the score of more
	than half of the live slices -- a kernel that read one table for the other would not pass"""
	runs = [(loc, len_t, stream) for n, loc, len_t, stream in L.exact_plan() if n == name and stream.startswith("shared")]
	assert {stream for _, _, stream in runs} == {"shared", "shared64"}
	for loc, len_t, stream in runs:
		c = L.corpus_of(stream)
		live = c["lens"] > 0
		s = L.gap_settings(len_t)[name]
		ref = L.oracle_exact(oracle, stream, name, loc, len_t)
		assert len(ref["sentence"]) == L.EXACT_MATCHES
		for i, sl in enumerate(ref["sentence"]):
			matched = slice_ids(c, int(sl))[ref["mapping"][i][ref["mapping"][i] >= 0]]
			assert len(matched) > len(set(matched.tolist())), (name, loc, int(sl))
		if name in L.SYMMETRIC:
			continue
		swapped = L.oracle_exact(oracle, stream, name, loc, len_t, gaps=(s.gap_t, s.gap_s))
		moved = (ref["all_scores"] != swapped["all_scores"])[live]
		print(f"{name} {LOCALITIES[loc]} {stream} len_t {len_t}: swapping w_s / w_t moves {int(moved.sum())} of {int(live.sum())} live slices")
		assert moved.mean() > 0.5, (name, loc, len_t, moved.mean())


@pytest.mark.parametrize("len_t", L.EXACT_LENS + (160,))
def test_expected_wt_tail(len_t):
	"""what each table is built to have is what the host's rule gives, and the tail branch is entered for len_t - tail columns at least"""
	S = L.gap_settings(len_t)
	listed = dict(sat1=1, sat2=2, sat8=8, sat9=9, sat10=10, sat_last=len_t - 1, last_differs=0, zigzag=0, tab_lin=0, aff_tab=9,
		lin0=0, lin_asym=0, lin_big=0, aff=0, aff0=0, aff_lin=0, csat2=2, csat8=8, csat9=9, csat10=10)
	# `steps` is constant over every three entries: the rule finds a tail of len_t - 1 or len_t - 2 unless len_t = 3 j + 1
	listed["steps"] = {65: 64, 80: 79, 129: 127, 160: 0}[len_t]
	for name, s in S.items():
		assert s.tail == listed[name] == L.wt_tail_rule(s.gap_s, s.gap_t, len_t), name
		assert 0 <= s.tail < len_t
		assert L.gap_mode(s.gap_s, s.gap_t) == (0 if name in L.LINEAR_SETTINGS else 1 if name in L.AFFINE_SETTINGS else 2)
		if L.kind_of(s.gap_s) == L.kind_of(s.gap_t) == "table":
			assert not (s.gap_s[1] == s.gap_t[1]).all(), name   # w_s != w_t
	assert {S[n].tail - 1 for n in ("sat8", "sat9", "sat10")} == {7, 8, 9}   # one candidate short of a trip of eight, a full trip, one more
	for name in L.CONCAVE_SETTINGS:   # strictly subadditive up to the tail and one step beyond: no two gaps stand in for one
		w = S[name].gap_t[1].astype(np.float64)
		assert all(w[k] < w[a] + w[k - a] for k in range(2, S[name].tail + 2) for a in range(1, k)), name
	for name, s in L.float_settings().items():
		assert s.tail == L.wt_tail_rule(s.gap_s, s.gap_t, len_t) < len_t, name


@pytest.mark.parametrize("name", [n for n in L.TABLE_SETTINGS + L.CONCAVE_SETTINGS if n not in ("last_differs", "zigzag", "tab_lin")])
def test_the_tail_decides_exact_scores(oracle, name):
	"""the exact runs of a setting: a tail moved one entry early moves scores, so the kernels' tail_max is not idle in them.  A tail of
	up to 10 tokens: gaps that long are everywhere -- over the setting's runs ten scores of slices of at most 64 tokens
	(vk_longq_kernel) and one of a longer slice (vk_longq_blocks_kernel) at the least; a tail of len_t - 1 or len_t - 2 costs
	otherwise only where nearly the whole query is one gap: one score at the least"""
	short = long_ = 0
	for _, loc, len_t, stream in [r for r in L.exact_plan() if r[0] == name]:
		s = L.gap_settings(len_t)[name]
		if s.tail == 0 or (stream.startswith("planted") and loc != L.GLOBAL):   # (the planted ties need no gap at all)
			continue
		lens = L.corpus_of(stream)["lens"]
		ref = L.oracle_exact(oracle, stream, name, loc, len_t)
		if s.tail == 1:   # (nothing before the first entry to move it to: lift the tail instead)
			w = s.gap_t[1].copy()
			w[2:] += 0.125
			moved_t = ("table", w)
		else:
			moved_t = L.truncated(s.gap_t, s.tail)
		other = L.oracle_exact(oracle, stream, name, loc, len_t, gaps=(s.gap_s, moved_t))
		moved = (ref["all_scores"] != other["all_scores"]) & (lens > 0)
		short, long_ = short + int((moved & (lens <= 64)).sum()), long_ + int((moved & (lens > 64)).sum())
		print(f"{name} {LOCALITIES[loc]} {stream} len_t {len_t} tail {s.tail}: moving the tail moves {int(moved.sum())} scores")
	if name in ("sat_last", "steps"):
		assert short + long_ >= 1, (name, short, long_)
	else:
		assert short >= 10 and long_ >= 1, (name, short, long_)


@pytest.mark.parametrize("d,len_t", L.FLOAT_CASES)
def test_float_corpora_are_sensitive(oracle, d, len_t):
	"""under GLOBAL (every query token is aligned or skipped) a tail one entry early, and w_s / w_t swapped, each move the oracle's score
	of more than half of the live slices by more than 2e-4 -- twice what the GPU module tolerates"""
	corpus, Xb, Qb = L.float_case(d, len_t)
	live = corpus["lens"] > 0

	def scores(gs, gt):
		return np.asarray(oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=d, sent_off=corpus["sent_off"], X=Xb, Q=Qb, locality=L.GLOBAL, gap_s=gs, gap_t=gt,
			max_matches=1, min_score=-1e9, want_all_scores=True, n_threads=8)["all_scores"], dtype=np.float64)[live]

	for name, s in L.float_settings().items():
		ref = scores(s.gap_s, s.gap_t)
		swapped = np.abs(scores(s.gap_t, s.gap_s) - ref) > 2e-4
		print(f"d {d} len_t {len_t} {name}: swapped tables move {int(swapped.sum())} of {len(ref)}")
		assert swapped.mean() > 0.5, (name, swapped.mean())
		if s.tail:
			early = np.abs(scores(s.gap_s, L.truncated(s.gap_t, s.tail)) - ref) > 2e-4
			print(f"d {d} len_t {len_t} {name}: a tail one entry early moves {int(early.sum())} of {len(ref)}")
			assert early.mean() > 0.5, (name, early.mean())
