"""-m gpu: operator chains on the cosine over contextual corpora (vk_corpus_set_contextual_sim_ops).

The reference of every check (contextual_chain_cases): the oracle only knows the clipped cosine, so the matrix of a chain is stated
around it -- T = clip(chain(raw)) with the unclipped canonical cosine of the token rows, the chain in numpy float32 exactly as
vectorian_amd/kernel.py states it, and no sim[id(t_j)][j] = 1 rewrite -- and handed to the oracle's contextual route as a
caller-supplied matrix (S_rows), which every algorithm and the tag weights read.

Corpora: about 350 slices of 3 .. 30 tokens; where the forms over longer slices matter (GAP 6, the wider strips of vk_score32_kernel)
seven more slices of 33 .. 64 tokens.  Without the feature every test here fails at its first call: the entry point does not exist."""

import ctypes as C

import numpy as np
import pytest

import bound_cases as bc
import contextual_chain_cases as cc
import route_cases as rc
import sim_ops_cases as sc
from helpers import assert_same_results
from vectorian_amd import alignment, synth
from vectorian_amd.corpus import Document
from vectorian_amd.embedding import ContextualEmbedding
from vectorian_amd.session import Session
from vectorian_amd.sim import Bias, CosineSim, EmbeddingTokenSim, ModifiedVectorSim, OptimizedSpanSim, Scale

pytestmark = pytest.mark.gpu

EXTRA = (33, 40, 47, 48, 56, 64, 64)
# name -> (d, precision, extra slices, seed): every width where the scoring kernel changes form -- nk32 = 2; a half-filled tail; the
# widths whose cosine runs specialised (300, 768: here the eight-deep generic form); fp32 rows at 64 and at 300 features
SPECS = {"d64": (64, "bf16", (), 7), "d64x": (64, "bf16", EXTRA, 9), "d100x": (100, "bf16", EXTRA, 11), "d300x": (300, "bf16", EXTRA, 15),
	"d768x": (768, "bf16", EXTRA, 17), "f64x": (64, "f32", EXTRA, 13), "f300": (300, "f32", (), 19)}
NARROW = ("d64", "d64x", "d100x", "f64x")   # d <= 100: the cases of the Threshold chain
LOCALITIES = ((0, 0.0), (1, -1e9), (2, -1e9))   # (locality, min_score)
LENS = (7, 16, 17, 32, 40, 64)   # 7 and 17 leave padded query columns: under (a) a lost mask shows as cells of 0.5


def exp5(n):
	return (1 - 2.0 ** (-np.arange(n) / 5)).astype(np.float32)


def gaps(name):
	return {"linear": (0.1, 0.05), "affine": (("affine", 0.2, 0.05), ("affine", 0.1, 0.02)), "exp5": (("table", exp5(513)), ("table", exp5(513)))}[name]


@pytest.fixture(scope="module")
def cases(hip, oracle):
	made = {}

	def get(name):
		if name not in made:
			d, precision, extra, seed = SPECS[name]
			made[name] = cc.Case(hip, oracle, d, extra=extra, seed=seed, precision=precision)
		return made[name]
	yield get
	for case in made.values():
		case.c.close()


def query_route(hip, c):
	lib = hip.lib()
	lib.vk_query_route.restype = C.c_int
	lib.vk_query_route.argtypes = [C.c_void_p, C.c_void_p]
	st = np.zeros(len(rc.STATE), dtype=np.int64)
	with c.lock:
		hip._check(lib.vk_query_route(c._h, st.ctypes.data))
	return dict(zip(rc.STATE, st.tolist()))


def batch_route(hip, c):
	lib = hip.lib()
	lib.vk_batch_state.restype = C.c_int
	lib.vk_batch_state.argtypes = [C.c_void_p, C.c_void_p]
	st = np.zeros(16, dtype=np.int64)
	with c.lock:
		hip._check(lib.vk_batch_state(c._h, st.ctypes.data))
	return int(st[0])


def check_alignment(case, c, Q, ops, loc, ms, gs, gt, k=9, off=None, T_of=None, **more):
	"""with and without tracebacks: ids, scores, mappings and the edges' similarities are the oracle's, bit for bit"""
	kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=k, min_score=ms)
	ref, T, raw = case.reference(Q, ops, **kw, **more)
	assert len(ref["score"]) > 0
	got = c.query(Q, q_normalize=False, **kw, **more)
	assert_same_results(got.trimmed(), ref, exact=True)
	for i in range(got.n):
		a = int(case.off[int(got.sentence[i])])
		for j in range(len(Q)):
			m = int(got.mapping[i, j])
			if m >= 0:
				want = T[a + m, j]
				assert got.edge_sim[i, j].view(np.uint32) == want.view(np.uint32), (i, j, got.edge_sim[i, j], want)
	noflow = c.query(Q, q_normalize=False, want_flow=False, **kw, **more)
	assert_same_results(noflow.trimmed(), ref, check_mapping=False, exact=True)
	return got, T, raw


def sweep(case, c, Q, ops, gap_names=("linear", "affine", "exp5")):
	plans = set()
	for gap in gap_names:
		gs, gt = gaps(gap)
		for loc, ms in LOCALITIES:
			check_alignment(case, c, Q, ops, loc, ms, gs, gt)
			plans.add(rc.PLAN[query_route(case.hip, c)["plan"]])
	return plans


@pytest.mark.parametrize("len_t", LENS)
@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_alignments_under_a_chain_are_the_oracles(cases, oracle, name, len_t):
	"""vk_score_kernel MODE 10 / 11 / 12 (at most 16 query tokens) and the chain forms of vk_score32_kernel (17 .. 64), every width
	where the form changes, three localities, linear / affine / table gaps (GAP 3 over slices of at most 32 tokens, GAP 6 beyond)"""
	for spec in SPECS:
		case = cases(spec)
		_, Q = case.query(len_t, seed=ord(name))
		ops = sc.chain(name)
		case.c.set_contextual_sim_ops(ops)
		plans = sweep(case, case.c, Q, ops)
		assert plans == ({"FUSED"} if len_t <= 16 else {"MULTI_BLOCK"}), (spec, plans)


@pytest.mark.parametrize("len_t", LENS)
def test_alignments_under_a_threshold(cases, oracle, len_t):
	"""chain (b) on the rows of at most 100 features: the scoring pass (matrix-pipe sums) and the restatement (canonical sums) differ by
	at most (d + 1) 2^-24 < 1e-5 per cell there, and pick_threshold asserts half a gap of 1e-5 around the threshold"""
	for spec in NARROW:
		case = cases(spec)
		_, Q = case.query(len_t, seed=ord("b"))
		ops = cc.chain_for("b", oracle, case, Q)
		case.c.set_contextual_sim_ops(ops)
		sweep(case, case.c, Q, ops)


@pytest.mark.parametrize("len_t", [7, 20, 40])
@pytest.mark.parametrize("name", ["e", "f"])
def test_transcendental_chains_within_the_transport_tolerance(cases, oracle, name, len_t):
	"""device powf / expf and numpy's differ by a few ulp per cell: below 1e-6 on a score normalised by len_t.  A cell off by an ulp can
	flip a tie of the traceback: no mapping check"""
	for spec in ("d64x", "d300x", "f64x"):
		case = cases(spec)
		_, Q = case.query(len_t, seed=ord(name))
		ops = sc.chain(name)
		case.c.set_contextual_sim_ops(ops)
		for gap in ("linear", "exp5"):
			gs, gt = gaps(gap)
			for loc, ms in LOCALITIES:
				kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=9, min_score=ms)
				ref, _, _ = case.reference(Q, ops, **kw)
				got = case.c.query(Q, q_normalize=False, **kw)
				assert_same_results(got.trimmed(), ref, check_mapping=False, exact=False, score_tol=2e-5, tie_tol=2e-5)


def test_the_order_of_operations(cases, oracle, hip):
	"""under (a) = (cos + 1) / 2 a cell of negative cosine is positive (the chain runs before the clip) and the padded query columns
	are 0, not 0.5; under (c) = 1 - cos a slice token that IS the query's token scores about 0, not 1 (no sim[id(t_j)][j] = 1 here)"""
	case = cases("d64")
	c = case.c
	_, Q = case.query(7, seed=3)
	ops = sc.chain("a")
	c.set_contextual_sim_ops(ops)
	T, raw = cc.chain_rows(oracle, case.X, Q, ops)
	negative = 0
	for loc, ms in LOCALITIES:
		got = c.query(Q, q_normalize=False, locality=loc, gap_s=0.05, gap_t=0.05, max_matches=9, min_score=ms, want_rows=True)
		assert got.n > 0
		for i in range(got.n):
			s = int(got.sentence[i])
			a, b = int(case.off[s]), int(case.off[s + 1])
			assert (got.sim_rows[i, :b - a, :7].view(np.uint32) == T[a:b].view(np.uint32)).all()
			assert (got.sim_rows[i, :b - a, 7:] == 0).all()           # the padding stays zero
			neg = raw[a:b] < 0
			negative += int(neg.sum())
			assert (got.sim_rows[i, :b - a, :7][neg] > 0).all()
	assert negative >= 20
	# (c): the query is a slice's own tokens under a little noise
	s = int(np.argmax(np.diff(case.off) >= 10))
	a = int(case.off[s])
	rng = np.random.default_rng(5)
	vec = case.raw_rows[a + 1:a + 8] / case.mag[a + 1:a + 8, None] + 0.02 * rng.standard_normal((7, case.d)).astype(np.float32)
	Q = case.rows(vec.astype(np.float32))
	ops = sc.chain("c")
	c.set_contextual_sim_ops(ops)
	T, raw = cc.chain_rows(oracle, case.X, Q, ops)
	got = c.query(Q, q_normalize=False, locality=0, gap_s=0.05, gap_t=0.05, max_matches=1, min_score=-1.0, want_rows=True, only_slices=np.array([s]))
	assert got.n == 1 and (got.sim_rows[0, :10, :7].view(np.uint32) == T[a:a + 10].view(np.uint32)).all()
	for j in range(7):
		assert raw[a + 1 + j, j] > 0.9 and got.sim_rows[0, 1 + j, j] < 0.1


# ---- transports

VARIANTS = {"nbow": (True, True, True), "bow/fast": (True, False, False), "nbow-onesided": (True, False, True),
	"nbow/distributed": (False, True, True), "distributed-onesided": (False, False, True), "distributed-bow": (False, False, False)}


@pytest.fixture(scope="module")
def transport_case(hip, oracle):
	case = cc.Case(hip, oracle, 64, extra=EXTRA, seed=23, magnitudes=True)
	yield case
	case.c.close()


@pytest.mark.parametrize("len_t", [7, 20])
@pytest.mark.parametrize("name", ["a", "b"])
def test_transports_under_a_chain(hip, oracle, transport_case, name, len_t):
	"""every RWMD variant, the full WMD and WRD, at most 16 query tokens (vk_score_kernel GAP 4 / 5 / 7) and beyond (vk_score32_kernel):
	the relaxed forms are restated on the host from the winners' canonical rows -- the oracle's floats --, the exact transports are
	held to the project's 2e-5; the winners' similarity rows are the cells of T"""
	case = transport_case
	c = case.c
	vec, Q = case.query(len_t, seed=ord(name) + 7)
	qmag = oracle.magnitudes(vec)
	ops = cc.chain_for(name, oracle, case, Q)
	c.set_contextual_sim_ops(ops)
	T, _ = cc.chain_rows(oracle, case.X, Q, ops)
	base = dict(max_matches=10, min_score=0.0)

	def rows_are_T(got):
		assert got.sim_rows is not None
		for i in range(got.n):
			a, b = int(case.off[int(got.sentence[i])]), int(case.off[int(got.sentence[i]) + 1])
			assert (got.sim_rows[i, :b - a, :len_t].view(np.uint32) == T[a:b].view(np.uint32)).all()
			assert (got.sim_rows[i, :b - a, len_t:] == 0).all()
	for variant, flags in VARIANTS.items():
		ref, _, _ = case.reference(Q, ops, algorithm=oracle.ALG_RWMD, rwmd=flags, want_all_scores=True, **base)
		got = c.query(vec, algorithm=hip.VK_ALG_RWMD, rwmd=flags, q_normalize=True, want_flow=True, **base)
		assert_same_results(got.trimmed(), ref, check_mapping=False, exact=True)
		rows_are_T(got)
		np.testing.assert_allclose(c.last_scores(), ref["all_scores"], atol=2e-5, rtol=0)   # the scoring pass itself, every slice
		noflow = c.query(vec, algorithm=hip.VK_ALG_RWMD, rwmd=flags, q_normalize=True, want_flow=False, **base)
		assert_same_results(noflow.trimmed(), ref, check_mapping=False, score_tol=2e-5, tie_tol=2e-5)
	for nbow in (False, True):
		kw = dict(rwmd=(False, False, nbow), wmd_full=True)
		ref, _, _ = case.reference(Q, ops, algorithm=oracle.ALG_RWMD, **kw, **base)
		got = c.query(vec, algorithm=hip.VK_ALG_RWMD, q_normalize=True, want_flow=True, **kw, **base)
		assert_same_results(got.trimmed(), ref, check_mapping=False, score_tol=2e-5, tie_tol=2e-5)
		rows_are_T(got)
		if nbow:
			for i in range(got.n):
				assert abs(float(got.plan[i].sum()) - 1.0) < 1e-4 and (got.plan[i] >= -1e-6).all()   # all of the normalised mass is moved
	for normalize in (True, False):
		ref, _, _ = case.reference(Q, ops, algorithm=oracle.ALG_WRD, wrd_normalize=normalize, X_mag=case.mag, Q_mag=qmag, **base)
		got = c.query(vec, algorithm=hip.VK_ALG_WRD, wrd_normalize=normalize, q_normalize=True, want_flow=True, **base)
		assert_same_results(got.trimmed(), ref, check_mapping=False, score_tol=2e-5, tie_tol=2e-5)
		rows_are_T(got)
		if normalize:
			for i in range(got.n):
				assert abs(float(got.plan[i].sum()) - 1.0) < 1e-4 and (got.plan[i] >= -1e-6).all()


# ---- routes

def test_no_bound_pass_and_no_span_kernel_under_a_chain(hip, oracle):
	"""a handle finalized under VK_BOUND_PASS=force has a shadow and takes the bound pass -- until it has a chain, whose output the
	shadow does not bound; a corpus of one-token slices under a one-token query takes the span kernel -- until it has a chain"""
	gs, gt = gaps("exp5")
	with bc.Env(VK_BOUND_PASS="force"):
		case = cc.Case(hip, oracle, 300, seed=31)   # (300-d bf16 rows: one of the two widths that have a shadow)
		c = case.c
		_, Q = case.query(7, seed=1)
		c.query(Q, q_normalize=False, locality=0, gap_s=gs, gap_t=gt, max_matches=9)
		assert rc.PLAN[query_route(hip, c)["plan"]] == "BOUNDED"
		for name in ("a", "d"):
			ops = sc.chain(name)
			c.set_contextual_sim_ops(ops)
			for loc, ms in LOCALITIES:
				check_alignment(case, c, Q, ops, loc, ms, gs, gt)
				state = query_route(hip, c)
				assert rc.PLAN[state["plan"]] == "FUSED" and rc.PASS[state["pass_short"]] == "FUSED"
		c.set_contextual_sim_ops([])
		c.query(Q, q_normalize=False, locality=0, gap_s=gs, gap_t=gt, max_matches=9)
		assert rc.PLAN[query_route(hip, c)["plan"]] == "BOUNDED"
		c.close()
	case = cc.Case(hip, oracle, 64, n=300, lo=1, hi=1, seed=33)
	c = case.c
	_, Q = case.query(1, seed=2)
	c.query(Q, q_normalize=False, locality=0, gap_s=0.1, gap_t=0.1, max_matches=9)
	assert rc.PLAN[query_route(hip, c)["plan"]] == "SPAN"
	for name in ("a", "c"):
		ops = sc.chain(name)
		c.set_contextual_sim_ops(ops)
		got, T, _ = check_alignment(case, c, Q, ops, 0, 0.0, 0.1, 0.1)
		state = query_route(hip, c)
		assert rc.PLAN[state["plan"]] == "FUSED" and rc.PASS[state["pass_short"]] == "FUSED"
		assert (got.score[:got.n].view(np.uint32) == np.sort(T[:, 0])[::-1][:got.n].view(np.uint32)).all()   # the score of a span IS its cell
	c.close()


# ---- the chain is state of the handle

def same(a, b):
	assert a.n == b.n
	for f in ("score", "raw_score", "sentence", "mapping", "edge_sim"):
		x, y = getattr(a, f)[:a.n], getattr(b, f)[:b.n]
		assert (x.view(np.uint32) == y.view(np.uint32)).all() if x.dtype == np.float32 else (x == y).all(), f


def test_views_filters_clearing_batches_tag_weights_and_boosts(hip, oracle):
	case = cc.Case(hip, oracle, 64, extra=EXTRA, seed=41, pos=True)
	c = case.c
	ops = sc.chain("a")
	kw = dict(q_normalize=False, locality=0, gap_s=0.1, gap_t=0.05, max_matches=9, min_score=0.0)
	okw = dict(locality=0, gap_s=0.1, gap_t=0.05, max_matches=9, min_score=0.0)
	_, Q = case.query(7, seed=9)
	plain = c.query(Q, **kw)
	c.set_contextual_sim_ops(ops)
	owner = c.query(Q, **kw)
	ref, T, _ = case.reference(Q, ops, **okw)
	assert_same_results(owner.trimmed(), ref, exact=True)
	assert not (owner.score[:owner.n] == plain.score[:plain.n]).all()
	# a view and a filtered corpus made after the chain was set: the owner's results (this filter drops nothing)
	view = c.view()
	same(view.query(Q, **kw), owner)
	filt = c.filtered(0, 0)
	same(filt.query(Q, **kw), owner)
	# ... after that each handle is set on its own
	view.set_contextual_sim_ops([])
	same(view.query(Q, **kw), plain)
	same(c.query(Q, **kw), owner)
	same(filt.query(Q, **kw), owner)
	view.close()
	filt.close()
	# a POS filter that drops tokens: the chain over the rows that stay, slices re-indexed
	keep = case.pos != 1
	new_index = np.concatenate(([0], np.cumsum(keep))).astype(np.int64)
	dropped = c.filtered(1 << 1, 0)
	Tf, _ = cc.chain_rows(oracle, case.X[keep], Q, ops)
	ref_f = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=case.d, sent_off=new_index[case.off], Q=Q, S_rows=[Tf], **okw)
	assert_same_results(dropped.query(Q, **kw).trimmed(), ref_f, exact=True)
	dropped.close()
	# batches run query by query through vk_query's code: route 1, vk_query's bits -- alignments and the relaxed WMD
	qs = [case.query(7 + i % 4, seed=20 + i)[1] for i in range(5)]
	outs = c.query_batch(qs, **kw)
	assert batch_route(hip, c) == 1
	for Q_i, out in zip(qs, outs):
		same(out, c.query(Q_i, **kw))
	tkw = dict(algorithm=hip.VK_ALG_RWMD, rwmd=(True, True, True), q_normalize=False, max_matches=10, min_score=0.0)
	qs = [case.query(10, seed=40 + i)[1] for i in range(9)]
	outs = c.query_batch(qs, **tkw)
	assert batch_route(hip, c) == 1
	for Q_i, out in zip(qs, outs):
		ref_t, _, _ = case.reference(Q_i, ops, algorithm=oracle.ALG_RWMD, rwmd=(True, True, True), max_matches=10, min_score=0.0)
		assert_same_results(out.trimmed(), ref_t, check_mapping=False, exact=True)
	# tag weights and a boost under a chain, at most 16 query tokens and beyond
	rng = np.random.default_rng(3)
	boost = rng.uniform(0.5, 1.5, size=len(case.off) - 1).astype(np.float32)
	for len_t in (7, 20):
		_, Q_t = case.query(len_t, seed=11)
		more = dict(tag_weights=rng.uniform(0.5, 1.5, size=len_t).astype(np.float32), q_pos=rng.integers(0, 4, size=len_t).astype(np.int8),
			pos_mismatch_penalty=0.3, similarity_threshold=0.2, boost=boost)
		for loc, ms in LOCALITIES:
			kq = dict(locality=loc, gap_s=0.1, gap_t=0.05, max_matches=9, min_score=ms)
			ref_w = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=case.d, sent_off=case.off, Q=Q_t, S_rows=[cc.chain_rows(oracle, case.X, Q_t, ops)[0]],
				pos_s=case.pos, **kq, **more)
			got = c.query(Q_t, q_normalize=False, **kq, **more)
			assert_same_results(got.trimmed(), ref_w, exact=True)
	# clearing the chain restores the unmodified results: those of a handle that never had one
	c.set_contextual_sim_ops([])
	same(c.query(Q, **kw), plain)
	fresh = case.handle()
	same(fresh.query(Q, **kw), plain)
	fresh.close()
	c.close()


def test_what_is_refused_and_with_which_words(hip, oracle):
	def status(call):
		with pytest.raises(hip.VkError) as e:
			call()
		return e.value.status, str(e.value)
	ops = sc.pairs(sc.chain("a"))
	# a corpus with a slice of 65 tokens: the chain may be set, the query is refused before anything is enqueued
	long_case = cc.Case(hip, oracle, 64, n=40, extra=(65,), seed=51)
	long_case.c.set_contextual_sim_ops(ops)
	_, Q = long_case.query(7, seed=1)
	for kw in (dict(), dict(algorithm=hip.VK_ALG_RWMD, rwmd=(True, True, True))):
		st, msg = status(lambda: long_case.c.query(Q, q_normalize=False, gap_s=0.1, gap_t=0.1, **kw))
		assert st == hip.VK_ERR_UNSUPPORTED and "operator chain" in msg and "slice of more than 64 tokens" in msg
	long_case.c.set_contextual_sim_ops([])
	assert long_case.c.query(Q, q_normalize=False, gap_s=0.1, gap_t=0.1).n > 0     # without the chain the corpus answers as before
	long_case.c.close()
	case = cc.Case(hip, oracle, 64, n=60, seed=53)
	c = case.c
	c.set_contextual_sim_ops(ops)
	# a query of 65 tokens
	_, Q65 = case.query(65, seed=2)
	st, msg = status(lambda: c.query(Q65, q_normalize=False, gap_s=0.1, gap_t=0.1))
	assert st == hip.VK_ERR_UNSUPPORTED and "operator chain" in msg and "query of more than 64 tokens" in msg
	# a query of 20 tokens the multi-block kernel does not take: affine gaps that open below their extension
	_, Q20 = case.query(20, seed=3)
	st, msg = status(lambda: c.query(Q20, q_normalize=False, gap_s=("affine", 0.2, 0.05), gap_t=("affine", -0.02, 0.05)))
	assert st == hip.VK_ERR_UNSUPPORTED and "operator chain" in msg and "multi-block kernel" in msg
	assert c.query(Q20, q_normalize=False, gap_s=("affine", 0.2, 0.05), gap_t=("affine", 0.1, 0.02)).n > 0
	# vk_corpus_set_sim_ops keeps refusing a contextual handle
	st, msg = status(lambda: c.set_sim_ops(ops))
	assert st == hip.VK_ERR_UNSUPPORTED and "CONTEXTUAL" in msg
	# a bad chain
	assert status(lambda: c.set_contextual_sim_ops([(hip.VK_SIMOP_BIAS, 0.1)] * 9))[0] == hip.VK_ERR_INVALID
	assert status(lambda: c.set_contextual_sim_ops([(6, 1.0)]))[0] == hip.VK_ERR_INVALID
	assert status(lambda: c.set_contextual_sim_ops([(hip.VK_SIMOP_SCALE, float("nan"))]))[0] == hip.VK_ERR_INVALID
	c.close()
	# a static handle
	st_corpus = synth.make_static_corpus(20, 3, 10, 50, 32, seed=3)
	s = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=32, n_tokens=len(st_corpus["tok_id"]), n_sentences=20, vocab_size=50)
	st, msg = status(lambda: s.set_contextual_sim_ops(ops))
	assert st == hip.VK_ERR_UNSUPPORTED and "vk_corpus_set_sim_ops" in msg
	s.close()
	# a handle under a span similarity, and the other way round
	sp = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=32, n_tokens=16, n_sentences=16)
	sp.set_span_sim(None, [(hip.VK_SIMOP_BIAS, 1.0)])
	st, msg = status(lambda: sp.set_contextual_sim_ops(ops))
	assert st == hip.VK_ERR_UNSUPPORTED and "span similarity" in msg
	sp.set_span_sim(None, [])
	sp.set_contextual_sim_ops(ops)
	st, msg = status(lambda: sp.set_span_sim(None, [(hip.VK_SIMOP_BIAS, 1.0)]))
	assert st == hip.VK_ERR_UNSUPPORTED and "vk_corpus_set_contextual_sim_ops" in msg
	sp.close()


# ---- the Python surface

def test_index_find_under_a_modified_vector_sim_over_a_contextual_embedding(hip, oracle):
	"""Index.find / find_many with ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5)) over a ContextualEmbedding: the slices, scores
	and flows of the oracle-backed double that states the chain around the oracle; a pos_filter gives a filtered corpus that carries the
	chain; debug = AllSlices(hook) states every slice from cells of the chain"""
	from vectorian_amd.index import AllSlices
	rng = np.random.default_rng(5)
	V, d = 300, 48
	E = synth.make_vocab(V, d)
	words = [f"w{i}" for i in range(V)]
	tags = ["NOUN", "VERB", "PRON", "ADJ"]
	docs = []
	for di in range(4):
		sents = [[words[i] for i in synth.zipf_ids(int(rng.integers(4, 30)), V, rng)] for _ in range(40)]
		pos = [[tags[int(w[1:]) % 4] for w in s] for s in sents]
		ids = [int(w[1:]) for s in sents for w in s]
		X = (E[ids] + 0.1 * rng.standard_normal((len(ids), d))).astype(np.float32)
		docs.append(Document(sents, pos=pos, tags=pos, unique_id=f"doc{di}", contextual_embeddings={"ctx": X}))
	emb = ContextualEmbedding("ctx", d, lambda tokens: E[[int(t[1:]) for t in tokens]])
	session = Session(docs, embeddings=[emb])
	vsim = ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5))
	sim = OptimizedSpanSim(EmbeddingTokenSim(emb, vsim), alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5)))
	gpu = session.partition("sentence").index(sim)
	cpu = session.partition("sentence").index(sim, corpus_factory=cc._double())
	assert gpu.metric_name == "ctx-((cosine + 1) * 0.5)" and cpu.metric_name == gpu.metric_name
	doc = session.documents[2]
	st = doc.spans["sentence"]["start"][7]
	texts = [" ".join(doc.tokens[st:st + 5]), "w3 w17 w4 w250 w2 w3", " ".join(doc.tokens[st:st + 22])]

	def key(res):
		return [(m.doc_index, m.slice_id, m.score) for m in res]
	for options in ({}, {"pos_filter": ["PRON"]}):
		for text in texts:
			a = gpu.find(text, n=8, min_score=-100.0, options=options)
			b = cpu.find(text, n=8, min_score=-100.0, options=options)
			assert len(a) > 0 and key(a) == key(b)
			for x, y in zip(a, b):
				assert (x.flow["target"] == y.flow["target"]).all() and (x.flow["dist"] == y.flow["dist"]).all()
		many = gpu.find_many(texts, n=8, min_score=-100.0, options=options)
		assert [key(r) for r in many] == [key(gpu.find(t, n=8, min_score=-100.0, options=options)) for t in texts]
	assert len(gpu._filtered) == 1
	# debug = AllSlices(hook): every slice, its similarity the cells of T and its score the oracle's alignment of them
	calls = []
	gpu.find(texts[1], n=4, min_score=-100.0, debug=AllSlices(lambda n_, d_: calls.append((n_, d_)), chunk=64))
	assert len(calls) == gpu.n_slices and all(n_ == "alignment" for n_, _ in calls)
	X = np.concatenate([dc.contextual_vectors("ctx") for dc in session.documents])
	Xb = oracle.normalize_rows_bf16(X)[0]
	Qb = oracle.normalize_rows_bf16(E[[int(t[1:]) for t in texts[1].split()]])[0]
	T, _ = cc.chain_rows(oracle, Xb, Qb, sc.chain("a"))
	w = alignment.smooth_gap_cost(5).costs(513)
	for g, (_, data) in enumerate(calls):
		a, b = int(gpu._slice_start[g]), int(gpu._slice_end[g])
		assert (data["similarity"].view(np.uint32) == T[a:b].view(np.uint32)).all()
		raw, mapping = oracle.align(T[a:b], 0, ("table", w), ("table", w))
		assert np.float32(data["score"]).view(np.uint32) == np.float32(raw).view(np.uint32) and (data["flow"]["target"] == mapping).all()
	# the plain cosine on the same session scores otherwise: the chain reached the device
	plain = session.partition("sentence").index(OptimizedSpanSim(EmbeddingTokenSim(emb, CosineSim()), alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5))))
	assert key(plain.find(texts[1], n=8, min_score=-100.0)) != key(gpu.find(texts[1], n=8, min_score=-100.0))
	plain.close()
	gpu.close()
