"""-m gpu: the p-norm distance and the improved sqrt-cosine as the VectorSim of a static corpus (vk_corpus_set_sim_source).

The reference of every check: the table is stated in numpy from the fp32 vectors in the order of vk_sim_src_host.h
(vector_sim_cases.source_matrix), then the chain (sim_ops_cases.apply_numpy), sim[id(t_j)][j] = 1 and the clip, and handed to the
oracle's contextual route as a caller-supplied matrix (S_rows), exactly as test_gpu_sim_ops.py does; transports go slice by slice
through oracle.rwmd / wmd / wrd.  Under such a source the table's cell is the canonical cell: chains of exactly rounded operations
-- (i) .. (iv) -- are held with ==, the powf / expf chains (v), (vi) within the project's 2e-5.  Every test asserts its condition
on the inputs: at least a third of the table's cells strictly inside (0, 1)."""

import numpy as np
import pytest

import vector_sim_cases as vc
from helpers import assert_same_results
from test_gpu_sim_ops import FORMS, LOCALITIES, gaps, rank, same
from vectorian_amd import alignment, synth
from vectorian_amd.corpus import Document
from vectorian_amd.embedding import StaticEmbedding
from vectorian_amd.session import Session
from vectorian_amd.sim import CosineSim, DistanceToSimilarity, EmbeddingTokenSim, ModifiedVectorSim, OptimizedSpanSim, PNormDistance, Scale

pytestmark = pytest.mark.gpu


class Case:
	"""a static corpus of raw standard_normal rows (magnitudes about sqrt(d)) on a handle that keeps them (a source is set before the
	rows are appended), and what the reference needs of it"""

	def __init__(self, hip, V, d, n, lo, hi, extra=(), seed=7, keep_magnitudes=False):
		st = synth.make_static_corpus(n, lo, hi, V, d, seed=seed)
		rng = np.random.default_rng(seed + 100)
		lens = list(np.diff(st["sent_off"])) + list(extra)
		self.ids = np.concatenate([st["tok_id"], synth.zipf_ids(int(sum(extra)), V, rng)]).astype(np.int32)
		self.off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
		self.V, self.d, self.hip, self.keep = V, d, hip, keep_magnitudes
		self.E = rng.standard_normal((V, d)).astype(np.float32)
		self.longest = int(max(lens))
		self.c = self.handle(hip.VK_SIMSRC_PNORM, 2.0)

	def handle(self, kind=None, arg=0.0):
		c = self.hip.Corpus(layout=self.hip.VK_LAYOUT_STATIC, d=self.d, n_tokens=len(self.ids), n_sentences=len(self.off) - 1, vocab_size=self.V,
			keep_magnitudes=self.keep)
		if kind is not None:
			c.set_sim_source(kind, arg)
		c.append_vectors(self.E, normalize=True)
		c.set_token_ids(self.ids)
		c.set_sentences(self.off)
		c.finalize()
		return c

	def query(self, len_t, seed, noise=0.15):
		"""as test_gpu_sim_ops.Case.query, on the raw vectors: len_t tokens quoted from the corpus, a repeated word, a word outside the
		vocabulary (id -1, a vector of its own), noise on every vector (noise = 0: the vocabulary's own vectors, as transports need them)"""
		rng = np.random.default_rng(1000 * len_t + seed)
		start = int(rng.integers(0, len(self.ids) - len_t))
		q_ids = self.ids[start:start + len_t].copy()
		q_ids[2] = q_ids[0]
		vec = self.E[q_ids] + np.float32(noise) * rng.standard_normal((len_t, self.d)).astype(np.float32)
		vec[2] = vec[0]
		q_ids[4] = -1
		vec[4] = rng.standard_normal(self.d).astype(np.float32)
		return q_ids.astype(np.int32), np.ascontiguousarray(vec, dtype=np.float32)

	def use(self, name, Q, c=None):
		"""chain (i) .. (vi) for this query on the handle; returns (source pair, operators)"""
		src, ops = vc.chain(name, self.E, Q)
		c = c or self.c
		c.set_sim_source(*vc.source_of(src))
		c.set_sim_ops(ops)
		return vc.source_of(src), ops


def reference(oracle, case, q_ids, Q, source, ops, **kw):
	T, mod = vc.table(case.E, Q, q_ids, source, ops)
	vc.assert_inside(T)
	Qb = synth.to_bf16_bits(synth.normalize_rows(Q))   # (the oracle reads its similarities from S_rows)
	ref = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=case.d, sent_off=case.off, Q=Qb, S_rows=[T[case.ids]], **kw)
	return ref, T, mod


def check_alignment(oracle, case, q_ids, Q, source, ops, loc, ms, gs, gt, exact=True, k=9):
	kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=k, min_score=ms)
	ref, T, _ = reference(oracle, case, q_ids, Q, source, ops, **kw)
	assert len(ref["score"]) > 0
	got = case.c.query(Q, q_token_ids=q_ids, **kw)
	noflow = case.c.query(Q, q_token_ids=q_ids, want_flow=False, **kw)
	if not exact:   # powf / expf: a cell off by an ulp can flip a tie of the traceback
		assert_same_results(got.trimmed(), ref, check_mapping=False, exact=False, score_tol=2e-5, tie_tol=2e-5)
		assert_same_results(noflow.trimmed(), ref, check_mapping=False, exact=False, score_tol=2e-5, tie_tol=2e-5)
		return got
	assert_same_results(got.trimmed(), ref, exact=True)
	for i in range(got.n):
		a = int(case.off[int(got.sentence[i])])
		for j in range(len(q_ids)):
			m = int(got.mapping[i, j])
			if m >= 0:
				want = T[case.ids[a + m], j]
				assert got.edge_sim[i, j].view(np.uint32) == want.view(np.uint32), (i, j, got.edge_sim[i, j], want)
	assert_same_results(noflow.trimmed(), ref, check_mapping=False, exact=True)
	return got


@pytest.fixture(scope="module")
def case_a(hip):
	case = Case(hip, V=500, d=64, n=350, lo=3, hi=30)
	yield case
	case.c.close()


@pytest.fixture(scope="module")
def case_b(hip):
	case = Case(hip, V=37, d=100, n=320, lo=3, hi=30, seed=11)
	yield case
	case.c.close()


@pytest.fixture(scope="module")
def case_c(hip):
	case = Case(hip, V=203, d=67, n=320, lo=3, hi=30, seed=17)
	yield case
	case.c.close()


@pytest.mark.parametrize("len_t", [7, 16, 17, 32, 40, 70])
@pytest.mark.parametrize("name", ["i", "ii", "iii", "iv", "v", "vi"])
def test_alignments_on_every_route_are_the_oracles(hip, oracle, case_a, case_b, case_c, name, len_t):
	"""fused, vk_score32, wide, vk_longq; all three localities; linear, affine and table gaps; V = 500 with d = 64, V = 37 (a partial
	last vocabulary tile) with d = 100 (a feature tail), and d = 67 (no multiple of 4: the four partial sums differ in length)"""
	for case in (case_a, case_b, case_c):
		q_ids, Q = case.query(len_t, seed=len(name))
		source, ops = case.use(name, Q)
		for gap in ("linear", "affine", "exp5"):
			gs, gt = gaps(gap, case.longest)
			for loc, ms in LOCALITIES:
				check_alignment(oracle, case, q_ids, Q, source, ops, loc, ms, gs, gt, exact=name not in ("v", "vi"))


@pytest.fixture(scope="module")
def long_cases(hip):
	cases = {600: Case(hip, V=500, d=64, n=300, lo=3, hi=30, extra=(70, 200, 600), seed=13),
		512: Case(hip, V=500, d=64, n=300, lo=3, hi=30, extra=(70, 200, 512), seed=13)}
	yield cases
	for case in cases.values():
		case.c.close()


@pytest.mark.parametrize("len_t", [10, 40, 70])
@pytest.mark.parametrize("name", ["i", "iii"])
def test_long_slices(hip, oracle, long_cases, name, len_t):
	"""slices of 70, 200 and 600 tokens among the short ones (vk_doc / vk_docw, the block form of vk_longq, and their restatement
	sites); queries of more than 64 tokens stop at slices of 512 tokens, so theirs is 512 long"""
	case = long_cases[512 if len_t > 64 else 600]
	q_ids, Q = case.query(len_t, seed=len(name) + 1)
	source, ops = case.use(name, Q)
	longs = set(range(len(case.off) - 4, len(case.off) - 1))
	seen = set()
	for gap in ("linear", "affine", "exp5"):
		gs, gt = gaps(gap, case.longest)
		for loc, ms in LOCALITIES:
			got = check_alignment(oracle, case, q_ids, Q, source, ops, loc, ms, gs, gt, k=12)
			seen |= longs & {int(s) for s in got.sentence[:got.n]}
	assert seen   # a long slice is among the winners somewhere (local alignments favour them)


@pytest.mark.parametrize("len_t", [7, 20])
@pytest.mark.parametrize("name", ["i", "iii"])
def test_transports(hip, oracle, name, len_t):
	"""all three RWMD variants, full WMD and WRD over a corpus with magnitudes; the winners' sim_rows are table rows bit for bit.  The
	7-token case is the padding check: nine padding columns whose distance to a vocabulary row is not zero"""
	case = Case(hip, V=500, d=64, n=350, lo=3, hi=30, seed=23, keep_magnitudes=True)
	c, E, ids, off = case.c, case.E, case.ids, case.off
	q_ids, qv = case.query(len_t, seed=ord(name[0]), noise=0.0)
	source, ops = case.use(name, qv)
	T, _ = vc.table(E, qv, q_ids, source, ops)
	vc.assert_inside(T)
	_, emag = oracle.normalize_rows_bf16(E)
	_, qmag = oracle.normalize_rows_bf16(qv)
	n = len(off) - 1
	forms = dict(FORMS, **{"rwmd 1:1 bow": ("rwmd", dict(rwmd=(True, False, False)))})
	for form, (alg, kw) in forms.items():
		values = np.empty(n, np.float32)
		for s in range(n):
			a, b = int(off[s]), int(off[s + 1])
			S = T[ids[a:b]]
			if alg == "wrd":
				raw = oracle.wrd(S, emag[ids[a:b]], qmag, normalize_magnitudes=True)
			elif kw.get("wmd_full"):
				raw = oracle.wmd(S, ids[a:b], q_ids, relaxed=False, injective=kw["rwmd"][0], symmetric=kw["rwmd"][1], normalize_bow=kw["rwmd"][2])
			else:
				raw = oracle.rwmd(S, ids[a:b], q_ids, injective=kw["rwmd"][0], symmetric=kw["rwmd"][1], normalize_bow=kw["rwmd"][2])
			values[s] = oracle.score(raw, len_t, len_t, 0.0, 1.0)
		ref = rank(values, 10, 0.0)
		h_alg = hip.VK_ALG_WRD if alg == "wrd" else hip.VK_ALG_RWMD
		got = c.query(qv, q_token_ids=q_ids, algorithm=h_alg, max_matches=10, min_score=0.0, want_flow=False, **kw)
		assert_same_results(got.trimmed(), ref, check_mapping=False, score_tol=2e-5, tie_tol=2e-5)
		if form == "rwmd 1:1":
			rows = c.query(qv, q_token_ids=q_ids, algorithm=h_alg, max_matches=10, min_score=0.0, want_flow=True, **kw)
			assert rows.sim_rows is not None
			assert_same_results(rows.trimmed(), ref, check_mapping=False, exact=True)
			for i in range(rows.n):
				a, b = int(off[int(rows.sentence[i])]), int(off[int(rows.sentence[i]) + 1])
				assert (rows.sim_rows[i, :b - a, :len_t].view(np.uint32) == T[ids[a:b]].view(np.uint32)).all()
				assert (rows.sim_rows[i, :b - a, len_t:] == 0).all()   # the padding columns
	c.close()


def test_the_order_of_operations(hip, oracle, case_a):
	"""under (i): a slice token that IS a query word reports similarity exactly 1.0 where the chain alone gives less (the rewrite runs
	after the chain), and a vocabulary row equal to the vector of a query word outside the vocabulary has distance exactly 0, hence
	similarity 1, with no rewrite"""
	case = case_a
	q_ids, Q = case.query(7, seed=3)
	w = int(case.ids[int(case.off[5])])   # the first word of slice 5 as the out-of-vocabulary token's vector
	Q[4] = case.E[w]
	source, ops = case.use("i", Q)
	T, mod = vc.table(case.E, Q, q_ids, source, ops)
	vc.assert_inside(T)
	assert vc.source_matrix(case.E[w:w + 1], Q[4:5], source)[0, 0] == 0 and mod[w, 4] == 1.0 and q_ids[4] == -1
	own = equal = 0
	for loc, ms in LOCALITIES:
		got = case.c.query(Q, q_token_ids=q_ids, locality=loc, gap_s=0.05, gap_t=0.05, max_matches=9, min_score=ms, want_rows=True)
		for i in range(got.n):
			s = int(got.sentence[i])
			a, b = int(case.off[s]), int(case.off[s + 1])
			rows = got.sim_rows[i, :b - a, :7]
			assert (rows.view(np.uint32) == T[case.ids[a:b]].view(np.uint32)).all()
			hit = case.ids[a:b] == w
			equal += int(hit.sum())
			assert (rows[hit, 4] == np.float32(1.0)).all()
			for j in range(7):
				m = int(got.mapping[i, j])
				if m >= 0 and case.ids[a + m] == q_ids[j]:
					own += 1
					assert got.edge_sim[i, j] == np.float32(1.0)
					assert mod[q_ids[j], j] < 1.0   # what the chain alone leaves of the cell: the noisy copy's distance is not 0
	assert own >= 3 and equal >= 1


def test_views_filters_and_batches_inherit_the_source(hip, oracle, case_a):
	case, c = case_a, case_a.c
	kw = dict(locality=0, gap_s=0.1, gap_t=0.05, max_matches=9, min_score=0.0)
	q_ids, Q = case.query(7, seed=9)
	source, ops = case.use("i", Q)
	owner = c.query(Q, q_token_ids=q_ids, **kw)
	ref, _, _ = reference(oracle, case, q_ids, Q, source, ops, **kw)
	assert_same_results(owner.trimmed(), ref, exact=True)
	bytes_with = c.device_bytes
	view, filt = c.view(), c.filtered(0, 0)
	same(view.query(Q, q_token_ids=q_ids, **kw), owner)
	same(filt.query(Q, q_token_ids=q_ids, **kw), owner)
	view.close()
	filt.close()
	# the handle counts its second copy of the rows: 64 bytes per feature block of 16 and row, zero tile included
	plain = case.handle()
	assert bytes_with - plain.device_bytes >= ((case.V + 15) // 16 + 1) * 1024 * ((case.d + 15) // 16)
	plain.close()
	# a batch of 4 relaxed-WMD queries runs query by query: the four calls' results
	qs = [case.query(7 + i, seed=20 + i, noise=0.0) for i in range(4)]
	case.use("i", qs[0][1])
	tkw = dict(algorithm=hip.VK_ALG_RWMD, rwmd=(True, True, True), max_matches=10, min_score=0.0)
	outs = c.query_batch([q for _, q in qs], token_ids=[i for i, _ in qs], **tkw)
	for (ids_i, Q_i), out in zip(qs, outs):
		one = c.query(Q_i, q_token_ids=ids_i, **tkw)
		assert out.n == one.n > 0
		assert (out.sentence[:out.n] == one.sentence[:one.n]).all() and (out.score[:out.n].view(np.uint32) == one.score[:one.n].view(np.uint32)).all()


def test_what_the_entry_point_refuses_on_a_live_handle(hip, case_a):
	def status(corpus, kind, arg=0.0):
		with pytest.raises(hip.VkError) as e:
			corpus.set_sim_source(kind, arg)
		return e.value.status, str(e.value)
	late = case_a.handle()   # never had a source: the rows are gone
	assert status(late, hip.VK_SIMSRC_PNORM, 2.0)[0] == hip.VK_ERR_STATE
	assert status(late, hip.VK_SIMSRC_SQRT_COSINE)[0] == hip.VK_ERR_STATE
	late.set_sim_source(hip.VK_SIMSRC_COSINE)
	fresh = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=8, n_tokens=4, n_sentences=1, vocab_size=4)
	fresh.append_vectors(np.eye(4, 8, dtype=np.float32))
	assert status(fresh, hip.VK_SIMSRC_PNORM, 1.0)[0] == hip.VK_ERR_STATE   # after the first append, before finalize
	fresh.close()
	ctx = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=16, n_tokens=32, n_sentences=2)
	st, msg = status(ctx, hip.VK_SIMSRC_PNORM, 2.0)
	assert st == hip.VK_ERR_UNSUPPORTED and "CONTEXTUAL" in msg
	ctx.set_sim_source(hip.VK_SIMSRC_COSINE)
	ctx.close()
	c = case_a.c
	for kind, arg in ((3, 0.0), (-1, 0.0), (hip.VK_SIMSRC_PNORM, 0.0), (hip.VK_SIMSRC_PNORM, -1.0), (hip.VK_SIMSRC_PNORM, float("inf")),
			(hip.VK_SIMSRC_PNORM, float("nan"))):
		assert status(c, kind, arg)[0] == hip.VK_ERR_INVALID, (kind, arg)
	late.close()


def test_the_cosine_handle_is_untouched(hip, case_a):
	"""a handle that never sets a source and one that sets VK_SIMSRC_COSINE (before the rows, and again after) answer alike"""
	never, cosine = case_a.handle(), case_a.handle(hip.VK_SIMSRC_COSINE)
	cosine.set_sim_source(hip.VK_SIMSRC_COSINE)
	assert never.device_bytes == cosine.device_bytes
	q_ids, Q = case_a.query(7, seed=5)
	for kw in (dict(locality=0, gap_s=0.1, gap_t=0.05), dict(algorithm=hip.VK_ALG_RWMD, rwmd=(True, True, True))):
		same(never.query(Q, q_token_ids=q_ids, max_matches=9, **kw), cosine.query(Q, q_token_ids=q_ids, max_matches=9, **kw))
	# ... and a handle that had a p-norm answers as they do once it is back on the cosine
	back = case_a.handle(hip.VK_SIMSRC_PNORM, 2.0)
	back.set_sim_source(hip.VK_SIMSRC_COSINE)
	same(never.query(Q, q_token_ids=q_ids, max_matches=9, locality=0, gap_s=0.1, gap_t=0.05), back.query(Q, q_token_ids=q_ids, max_matches=9, locality=0, gap_s=0.1, gap_t=0.05))
	for h in (never, cosine, back):
		h.close()


def test_index_find_many_is_find_under_a_p_norm(hip):
	"""Index.find / find_many through Session under ModifiedVectorSim(PNormDistance(2), Scale(s), DistanceToSimilarity()): the quoted
	sentence wins with score 1, a view answers as the owner, the plain cosine scores otherwise"""
	rng = np.random.default_rng(5)
	V, d = 300, 48
	E = rng.standard_normal((V, d)).astype(np.float32)
	words = [f"w{i}" for i in range(V)]
	docs = [Document([[words[i] for i in synth.zipf_ids(int(rng.integers(4, 30)), V, rng)] for _ in range(40)], unique_id=f"doc{di}") for di in range(4)]
	emb = StaticEmbedding("toy-48", words, E)
	session = Session(docs, embeddings=[emb])
	s = float(1 / (2 * np.sqrt(2 * d)))
	vsim = ModifiedVectorSim(PNormDistance(2), Scale(s), DistanceToSimilarity())
	gap = alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5))
	gpu = session.partition("sentence").index(OptimizedSpanSim(EmbeddingTokenSim(emb, vsim), gap))
	assert gpu.metric_name == f"toy-48-(1 - (p-norm(2) * {s}))"
	doc = session.documents[2]
	st, en = doc.spans["sentence"]["start"][7], doc.spans["sentence"]["end"][7]
	texts = [" ".join(doc.tokens[st:en]), "w3 w17 w4 w250 w2 w3", " ".join(doc.tokens[st:st + 22])]

	def key(res):
		return [(m.doc_index, m.slice_id, m.score) for m in res]
	best = gpu.find(texts[0], n=8, min_score=-100.0)
	assert (best[0].doc_index, best[0].slice_id) == (2, 7) and best[0].score == 1.0 and 0 < best[7].score < 1
	many = gpu.find_many(texts, n=8, min_score=-100.0)
	assert [key(r) for r in many] == [key(gpu.find(t, n=8, min_score=-100.0)) for t in texts]
	plain = session.partition("sentence").index(OptimizedSpanSim(EmbeddingTokenSim(emb, CosineSim()), gap))
	assert key(plain.find(texts[1], n=8, min_score=-100.0)) != key(gpu.find(texts[1], n=8, min_score=-100.0))
	plain.close()
	gpu.close()
