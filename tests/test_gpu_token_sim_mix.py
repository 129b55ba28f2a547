"""-m gpu: token similarity combinators over several static embeddings (vk_corpus_set_sim_mix).

The reference of every check: each operand's table is stated in numpy -- sim_ops_cases.chain_table for a cosine operand,
vector_sim_cases.table for a source operand -- the tables are combined with the reference's own numpy call
(vectorian_amd.modifier.*.__call__, which mirrors vectorian/sim/modifier.py) and handed to the oracle's contextual route as a
caller-supplied matrix (S_rows); transports go slice by slice through oracle.rwmd / wmd.  On a mixed handle the table's cell is the
canonical cell of every route: operands of exactly rounded operations are held with == on ids, scores, mappings, edge_sim and
sim_rows, a powf operand within the project's 2e-5 and without a mapping check.  sim_mix_cases.tables asserts the conditions on the
inputs with every table it states; tests/test_sim_mix_backend.py asserts all three on the CPU."""

import numpy as np
import pytest

import sim_mix_cases as mc
import sim_ops_cases as sc
import vector_sim_cases as vc
from helpers import assert_same_results
from sim_mix_backend import MixOracleCorpus
from test_gpu_sim_ops import FORMS, LOCALITIES, gaps, rank, same
from vectorian_amd import alignment, synth
from vectorian_amd.corpus import Document
from vectorian_amd.embedding import StaticEmbedding
from vectorian_amd.modifier import MaximumTokenSimilarity, MinimumTokenSimilarity, MixedTokenSimilarity
from vectorian_amd.session import Session
from vectorian_amd.sim import (Bias, CosineSim, DistanceToSimilarity, EmbeddingTokenSim, ModifiedVectorSim, OptimizedSpanSim, PNormDistance, Scale,
	Threshold)

pytestmark = pytest.mark.gpu


class Handle:
	"""a case of sim_mix_cases on the device: the mixed handle and what the reference needs of it"""

	def __init__(self, hip, name, extra=(), pos=False, precision="bf16"):
		self.corpus, self.combo, self.mix = mc.case(name, extra)
		self.ops_of = mc.operands(self.combo, self.corpus.dims)
		self.exact = mc.EXACT[self.combo]
		self.hip, self.precision = hip, precision
		self.pos = np.random.default_rng(5).integers(0, 4, size=len(self.corpus.ids)).astype(np.int8) if pos else None
		self.c = self.handle()

	def handle(self, mixed=True):
		k, hip = self.corpus, self.hip
		c = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=k.dims[0], n_tokens=len(k.ids), n_sentences=len(k.off) - 1, vocab_size=k.V, precision=self.precision)
		src, ops = self.ops_of[0]
		if mixed:
			mc.set_up(c, self.mix, k.dims, self.ops_of)
			for i in range(1, len(k.dims)):
				c.append_operand_vectors(i, k.E[i][:k.V // 2], normalize=True)   # (in two appends)
				c.append_operand_vectors(i, k.E[i][k.V // 2:], normalize=True)
		if src is not None:
			c.set_sim_source(*vc.source_of(src))
		c.append_vectors(k.E[0], normalize=True)
		c.set_sim_ops(ops)
		c.set_token_ids(k.ids)
		if self.pos is not None:
			c.set_token_pos(self.pos)
		c.set_sentences(k.off)
		c.finalize()
		return c

	def tables(self, oracle, q_ids, Qs):
		return mc.tables(oracle, self.corpus, q_ids, Qs, self.ops_of, self.mix)

	def reference(self, oracle, q_ids, Qs, **kw):
		T, each = self.tables(oracle, q_ids, Qs)
		k = self.corpus
		ref = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=k.dims[0], sent_off=k.off, Q=oracle.normalize_rows_bf16(Qs[0])[0], S_rows=[T[k.ids]], **kw)
		return ref, T

	def query(self, q_ids, Qs, c=None, **kw):
		return (c or self.c).query(Qs[0], q_operand_vectors=Qs[1:], q_token_ids=q_ids, **kw)


def check_alignment(oracle, h, q_ids, Qs, loc, ms, gs, gt, k=9, **more):
	"""with and without tracebacks: ids, scores, mappings and the edges' similarities are the oracle's"""
	kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=k, min_score=ms)
	ref, T = h.reference(oracle, q_ids, Qs, **kw, **{"pos_s" if n == "pos" else n: v for n, v in more.items()})
	assert len(ref["score"]) > 0
	hip_more = {n: v for n, v in more.items() if n != "pos"}
	got = h.query(q_ids, Qs, **kw, **hip_more)
	noflow = h.query(q_ids, Qs, want_flow=False, **kw, **hip_more)
	if not h.exact:   # powf: a cell off by an ulp can flip a tie of the traceback
		assert_same_results(got.trimmed(), ref, check_mapping=False, exact=False, score_tol=2e-5, tie_tol=2e-5)
		assert_same_results(noflow.trimmed(), ref, check_mapping=False, exact=False, score_tol=2e-5, tie_tol=2e-5)
		return got, ref
	assert_same_results(got.trimmed(), ref, exact=True)
	for i in range(got.n):
		a = int(h.corpus.off[int(got.sentence[i])])
		for j in range(len(q_ids)):
			m = int(got.mapping[i, j])
			if m >= 0:
				want = T[h.corpus.ids[a + m], j]
				assert got.edge_sim[i, j].view(np.uint32) == want.view(np.uint32), (i, j, got.edge_sim[i, j], want)
	assert_same_results(noflow.trimmed(), ref, check_mapping=False, exact=True)
	return got, ref


@pytest.fixture(scope="module")
def handles(hip):
	made = {}

	def get(name, **kw):
		key = (name, tuple(sorted(kw.items())))
		if key not in made:
			made[key] = Handle(hip, name, **kw)
		return made[key]
	yield get
	for h in made.values():
		h.c.close()


@pytest.mark.parametrize("len_t", mc.QUERY_LENGTHS)
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_alignments_on_every_route_are_the_oracles(hip, oracle, handles, name, len_t):
	"""fused, vk_score32, wide, vk_longq; the localities, a min_score above 0; linear, affine and table gaps; V = 500 and V = 37 (a
	partly empty workgroup of the table kernels); operand widths (64, 100), (67, 300) and (32, 67, 100); queries of 7 (nine padding
	columns), 16, 17 (two tiles), 40 and 70 tokens"""
	h = handles(name)
	q_ids, Qs = h.corpus.query(len_t, seed=mc.QUERY_SEED)
	for gap in ("linear", "affine", "exp5"):
		gs, gt = gaps(gap, h.corpus.longest)
		for loc, ms in LOCALITIES:
			_, ref = check_alignment(oracle, h, q_ids, Qs, loc, ms, gs, gt)
			if loc == 0:
				# ... and under a min_score above 0: between the reference's fourth and fifth best score, which ends the result set there
				best = ref["score"]
				assert len(best) == 9 and best[3] > best[5] > 0
				cut, _ = check_alignment(oracle, h, q_ids, Qs, loc, float((np.float64(best[3]) + np.float64(best[5])) / 2), gs, gt)
				assert 4 <= cut.n <= 5


@pytest.mark.parametrize("len_t", [10, 40, 70])
@pytest.mark.parametrize("name", ["tp-avg-int", "three-max"])
def test_long_slices(hip, oracle, handles, name, len_t):
	"""slices of about 100 and 600 tokens among the short ones (vk_doc / vk_docw, the block form of vk_longq, and their restatement
	sites); queries of more than 64 tokens stop at slices of 512 tokens, so theirs is 512 long"""
	h = handles(name, extra=(100, 512) if len_t > 64 else (100, 600))
	q_ids, Qs = h.corpus.query(len_t, seed=5)
	longs = set(range(len(h.corpus.off) - 3, len(h.corpus.off) - 1))
	seen = set()
	for gap in ("linear", "affine", "exp5"):
		gs, gt = gaps(gap, h.corpus.longest)
		for loc, ms in LOCALITIES:
			got, _ = check_alignment(oracle, h, q_ids, Qs, loc, ms, gs, gt, k=12)
			seen |= longs & {int(s) for s in got.sentence[:got.n]}
	assert seen   # a long slice is among the winners somewhere (local alignments favour them)


@pytest.mark.parametrize("len_t", [7, 20])
@pytest.mark.parametrize("name", ["aa-max", "cc-avg-int-v37", "three-avg-float-v37"])
def test_transports(hip, oracle, handles, name, len_t):
	"""the relaxed WMD in its variants and the full WMD; the winners' sim_rows are the combined table's rows bit for bit.  Word
	Rotator's Distance is refused: the reference leaves a combinator's magnitudes unwritten"""
	h = handles(name)
	k = h.corpus
	q_ids, Qs = k.query(len_t, seed=11, noise=0.0)
	T, _ = h.tables(oracle, q_ids, Qs)
	n = len(k.off) - 1
	forms = dict({f: v for f, v in FORMS.items() if f != "wrd"}, **{"rwmd 1:1 bow": ("rwmd", dict(rwmd=(True, False, False)))})
	for form, (alg, kw) in forms.items():
		values = np.empty(n, np.float32)
		for s in range(n):
			a, b = int(k.off[s]), int(k.off[s + 1])
			S = T[k.ids[a:b]]
			if kw.get("wmd_full"):
				raw = oracle.wmd(S, k.ids[a:b], q_ids, relaxed=False, injective=kw["rwmd"][0], symmetric=kw["rwmd"][1], normalize_bow=kw["rwmd"][2])
			else:
				raw = oracle.rwmd(S, k.ids[a:b], q_ids, injective=kw["rwmd"][0], symmetric=kw["rwmd"][1], normalize_bow=kw["rwmd"][2])
			values[s] = oracle.score(raw, len_t, len_t, 0.0, 1.0)
		ref = rank(values, 10, 0.0)
		got = h.query(q_ids, Qs, algorithm=hip.VK_ALG_RWMD, max_matches=10, min_score=0.0, want_flow=False, **kw)
		assert_same_results(got.trimmed(), ref, check_mapping=False, score_tol=2e-5, tie_tol=2e-5)
		if form == "rwmd 1:1":
			rows = h.query(q_ids, Qs, algorithm=hip.VK_ALG_RWMD, max_matches=10, min_score=0.0, want_flow=True, **kw)
			assert rows.sim_rows is not None
			assert_same_results(rows.trimmed(), ref, check_mapping=False, exact=True)
			for i in range(rows.n):
				a, b = int(k.off[int(rows.sentence[i])]), int(k.off[int(rows.sentence[i]) + 1])
				assert (rows.sim_rows[i, :b - a, :len_t].view(np.uint32) == T[k.ids[a:b]].view(np.uint32)).all()
				assert (rows.sim_rows[i, :b - a, len_t:] == 0).all()   # the padding columns
	with pytest.raises(hip.VkError) as e:
		h.query(q_ids, Qs, algorithm=hip.VK_ALG_WRD, max_matches=10)
	assert e.value.status == hip.VK_ERR_UNSUPPORTED and "magnitudes" in str(e.value)


@pytest.mark.parametrize("len_t", [7, 20])
def test_tag_weights(hip, oracle, handles, len_t):
	"""the tag-weighted similarity and a submatch weight read the mixed cell like any other"""
	h = handles("tp-avg-int", pos=True)
	q_ids, Qs = h.corpus.query(len_t, seed=13)
	rng = np.random.default_rng(len_t)
	tw = rng.choice([0.5, 1.0, 2.0], size=len_t).astype(np.float32)
	q_pos = rng.integers(0, 4, size=len_t).astype(np.int8)
	for loc, ms in LOCALITIES:
		check_alignment(oracle, h, q_ids, Qs, loc, ms, 0.1, 0.05, tag_weights=tw, q_pos=q_pos, pos_mismatch_penalty=0.25, similarity_threshold=0.2, pos=h.pos)
	kw = dict(locality=0, gap_s=0.1, gap_t=0.05, max_matches=9, min_score=0.0, submatch_weight=0.5)
	ref, _ = h.reference(oracle, q_ids, Qs, **kw)
	assert_same_results(h.query(q_ids, Qs, **kw).trimmed(), ref, exact=True)


def test_views_filters_and_batches_inherit_the_mix(hip, oracle, handles):
	h = handles("tp-avg-int")
	c = h.c
	kw = dict(locality=0, gap_s=0.1, gap_t=0.05, max_matches=9, min_score=0.0)
	q_ids, Qs = h.corpus.query(7, seed=9)
	owner = h.query(q_ids, Qs, **kw)
	ref, _ = h.reference(oracle, q_ids, Qs, **kw)
	assert_same_results(owner.trimmed(), ref, exact=True)
	bytes_with = c.device_bytes
	view, filt = c.view(), c.filtered(0, 0)
	same(h.query(q_ids, Qs, c=view, **kw), owner)
	same(h.query(q_ids, Qs, c=filt, **kw), owner)
	view.close()
	filt.close()
	# the handle counts the operand's tiles and, under its p-norm, the fp32 copy of its rows (zero tile included)
	plain = h.handle(mixed=False)
	k = h.corpus
	tiles, d1 = (k.V + 15) // 16 + 1, k.dims[1]
	assert bytes_with - plain.device_bytes >= tiles * ((d1 + 15) // 16 * 16 * 32 + (d1 + 15) // 16 * 1024)
	# ... and a handle without the mix scores otherwise: the other operand reached the device
	alone = plain.query(Qs[0], q_token_ids=q_ids, **kw)
	assert not (alone.n == owner.n and (alone.score[:alone.n] == owner.score[:owner.n]).all())
	plain.close()
	# batches run query by query, each with its own operand rows: 4 relaxed-WMD queries and 5 alignments of different lengths
	for tkw, noise in ((dict(algorithm=hip.VK_ALG_RWMD, rwmd=(True, True, True), max_matches=10, min_score=0.0), 0.0), (kw, 0.15)):
		qs = [h.corpus.query(7 + 3 * i, seed=20 + i, noise=noise) for i in range(5)]
		outs = c.query_batch([Q[0] for _, Q in qs], token_ids=[i for i, _ in qs], q_operand_vectors=[Q[1:] for _, Q in qs], **tkw)
		for (ids_i, Q_i), out in zip(qs, outs):
			one = h.query(ids_i, Q_i, **tkw)
			assert out.n == one.n > 0
			assert (out.sentence[:out.n] == one.sentence[:one.n]).all() and (out.score[:out.n].view(np.uint32) == one.score[:one.n].view(np.uint32)).all()


def test_operand_rows_are_per_query_state(hip, handles):
	"""a query without its operand rows, or with rows of another length, ends with VK_ERR_STATE; rows left by a failed query do not
	reach the next one"""
	h = handles("aa-max")
	q_ids, Qs = h.corpus.query(7, seed=9)
	kw = dict(locality=0, gap_s=0.1, gap_t=0.05, max_matches=9, min_score=0.0)
	good = h.query(q_ids, Qs, **kw)
	with pytest.raises(hip.VkError) as e:
		h.c.query(Qs[0], q_token_ids=q_ids, **kw)
	assert e.value.status == hip.VK_ERR_STATE and "operand 1" in str(e.value)
	with pytest.raises(hip.VkError) as e:
		h.c.query(Qs[0], q_operand_vectors=[Qs[1][:5]], q_token_ids=q_ids, **kw)
	assert e.value.status == hip.VK_ERR_STATE and "5 rows" in str(e.value)
	with pytest.raises(hip.VkError) as e:
		h.c.query(Qs[0], q_token_ids=q_ids, **kw)   # the five rows are gone
	assert e.value.status == hip.VK_ERR_STATE
	same(h.query(q_ids, Qs, **kw), good)


def test_what_the_entry_points_refuse_on_a_live_handle(hip, handles):
	def status(call, *args):
		with pytest.raises(hip.VkError) as e:
			call(*args)
		return e.value.status, str(e.value)
	c = handles("aa-max").c
	assert status(c.set_sim_mix, hip.VK_SIMMIX_MAXIMUM, 2)[0] == hip.VK_ERR_STATE   # after the rows
	assert status(c.set_sim_operand, 1, 50)[0] == hip.VK_ERR_STATE                   # another width
	assert status(c.set_sim_operand, 1, 100, (hip.VK_SIMSRC_PNORM, 2.0))[0] == hip.VK_ERR_STATE   # it kept no unmodified rows
	assert status(c.set_sim_operand, 2, 100)[0] == hip.VK_ERR_INVALID and status(c.set_sim_operand, 0, 64)[0] == hip.VK_ERR_INVALID
	assert status(c.set_sim_operand, 1, 100, None, [(9, 1.0)])[0] == hip.VK_ERR_INVALID
	fresh = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=8, n_tokens=4, n_sentences=1, vocab_size=4)
	for kind, n, w in ((3, 2, [1, 1]), (hip.VK_SIMMIX_NONE, 2, [1, 1]), (hip.VK_SIMMIX_AVERAGE, 1, [1]), (hip.VK_SIMMIX_AVERAGE, 5, [1] * 5),
			(hip.VK_SIMMIX_AVERAGE, 2, None), (hip.VK_SIMMIX_AVERAGE, 2, [1, -1]), (hip.VK_SIMMIX_AVERAGE, 2, [float("nan"), 1]), (hip.VK_SIMMIX_AVERAGE, 2, [0, 0])):
		assert status(fresh.set_sim_mix, kind, n, w)[0] == hip.VK_ERR_INVALID, (kind, n, w)
	fresh._operand_d = {}
	assert status(fresh.set_sim_operand, 1, 8)[0] == hip.VK_ERR_STATE   # no combinator
	fresh.set_sim_mix(hip.VK_SIMMIX_AVERAGE, 2, [1, 3])
	assert status(fresh.set_sim_operand, 1, 2000, (hip.VK_SIMSRC_PNORM, 2.0))[0] == hip.VK_ERR_UNSUPPORTED   # wider than 1024 under a source
	fresh.set_sim_operand(1, 12)
	fresh.append_vectors(np.eye(4, 8, dtype=np.float32))
	fresh.append_operand_vectors(1, np.ones((3, 12), np.float32))
	fresh.set_token_ids(np.arange(4))
	fresh.set_sentences(np.array([0, 4]))
	st, msg = status(fresh.finalize)
	assert st == hip.VK_ERR_STATE and "3 of 4" in msg   # the operand lacks a row
	assert status(fresh.append_operand_vectors, 1, np.ones((2, 12), np.float32))[0] == hip.VK_ERR_INVALID   # more than declared
	fresh.append_operand_vectors(1, np.ones((1, 12), np.float32))
	fresh.finalize()
	fresh.close()
	ctx = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=16, n_tokens=32, n_sentences=2)
	st, msg = status(ctx.set_sim_mix, hip.VK_SIMMIX_MAXIMUM, 2)
	assert st == hip.VK_ERR_UNSUPPORTED and "CONTEXTUAL" in msg
	ctx.close()


def test_fp32_rows(hip, oracle):
	"""a handle of fp32 unit rows: the canonical table kernel's fp32 form, held against the combination of the oracle's fp32 cosines
	within the transport tolerance (the oracle states no chain around its fp32 cosine: the operands are plain)"""
	h = Handle(hip, "aa-max", precision="f32")
	h.c.set_sim_ops([])
	h.c.set_sim_operand(1, h.corpus.dims[1], None, [])
	k = h.corpus
	q_ids, Qs = k.query(20, seed=3)
	each = []
	for E, Q in zip(k.E, Qs):
		t = oracle.sim_f32(oracle.normalize_rows(E), oracle.normalize_rows(Q))
		t[sc.rewrite_mask(k.V, q_ids)] = 1.0
		each.append(np.clip(t, 0, 1).astype(np.float32))
	T = np.maximum(each[0], each[1])
	kw = dict(locality=0, gap_s=0.1, gap_t=0.05, max_matches=9, min_score=0.0)
	ref = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=k.dims[0], sent_off=k.off, Q=oracle.normalize_rows_bf16(Qs[0])[0], S_rows=[T[k.ids]], **kw)
	got = h.query(q_ids, Qs, **kw)
	assert_same_results(got.trimmed(), ref, check_mapping=False, exact=False, score_tol=2e-5, tie_tol=2e-5)
	h.c.close()


# ---- the Python surface

def test_index_find_and_find_many_under_the_combinators(hip):
	"""Index.find / find_many through Session: MixedTokenSimilarity with int weights, MaximumTokenSimilarity and MinimumTokenSimilarity
	over two static embeddings, against the same index on the oracle-backed double (sim_mix_backend.MixOracleCorpus) -- slices, scores
	and flows; a pos_filter gives a filtered corpus that carries the mix; "minimum" returns the MAXIMUM's result set"""
	rng = np.random.default_rng(5)
	V, d1, d2 = 300, 48, 100
	words = [f"w{i}" for i in range(V)]
	tags = ["NOUN", "VERB", "PRON", "ADJ"]
	docs = []
	for di in range(4):
		sents = [[words[i] for i in synth.zipf_ids(int(rng.integers(4, 30)), V, rng)] for _ in range(40)]
		pos = [[tags[int(w[1:]) % 4] for w in s] for s in sents]
		docs.append(Document(sents, pos=pos, tags=pos, unique_id=f"doc{di}"))
	e1 = StaticEmbedding("toy-48", words, rng.standard_normal((V, d1)).astype(np.float32))
	e2 = StaticEmbedding("toy-100", words, rng.standard_normal((V, d2)).astype(np.float32))
	session = Session(docs, embeddings=[e1, e2])
	first = EmbeddingTokenSim(e1, ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5), Threshold(0.47)))
	second = EmbeddingTokenSim(e2, ModifiedVectorSim(PNormDistance(2), Scale(float(1 / (2 * np.sqrt(2 * d2)))), DistanceToSimilarity()))
	gap = alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5))
	doc = session.documents[2]
	st = doc.spans["sentence"]["start"][7]
	texts = [" ".join(doc.tokens[st:st + 5]), "w3 w17 w4 w250 w2 w3", " ".join(doc.tokens[st:st + 22])]

	def key(res):
		return [(m.doc_index, m.slice_id, m.score) for m in res]
	results = {}
	for label, token_sim in (("mixed", MixedTokenSimilarity([first, second], [2, 1])), ("maximum", MaximumTokenSimilarity([first, second])),
			("minimum", MinimumTokenSimilarity([first, second]))):
		sim = OptimizedSpanSim(token_sim, gap)
		gpu = session.partition("sentence").index(sim)
		cpu = session.partition("sentence").index(sim, corpus_factory=MixOracleCorpus)
		assert gpu.metric_name == token_sim.name
		for options in ({}, {"pos_filter": ["PRON"]}):
			for text in texts:
				a = gpu.find(text, n=8, min_score=-100.0, options=options)
				b = cpu.find(text, n=8, min_score=-100.0, options=options)
				assert key(a) == key(b) and len(a) == 8
				for x, y in zip(a, b):
					assert (x.flow["target"] == y.flow["target"]).all() and (x.flow["dist"] == y.flow["dist"]).all()
			many = gpu.find_many(texts, n=8, min_score=-100.0, options=options)
			assert [key(r) for r in many] == [key(gpu.find(t, n=8, min_score=-100.0, options=options)) for t in texts]
		assert len(gpu._filtered) == 1
		results[label] = [key(gpu.find(t, n=8, min_score=-100.0)) for t in texts]
		gpu.close()
	assert results["minimum"] == results["maximum"] != results["mixed"]
	# operand 0 alone on the same session scores otherwise: the second embedding reached the device
	alone = session.partition("sentence").index(OptimizedSpanSim(first, gap))
	assert key(alone.find(texts[1], n=8, min_score=-100.0)) != results["maximum"][1]
	alone.close()
