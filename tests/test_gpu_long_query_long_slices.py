"""-m gpu: queries of 65 .. 512 tokens over corpora that hold slices of 65 .. 512 tokens (VK_ERR_UNSUPPORTED until this file came:
vk_validate_query refused such a query as soon as one slice had more than 64 tokens).  The block form of vk_longq_kernel takes
those slices -- column blocks of 64 slice tokens behind a border column, DESIGN 8.1 -- after the pass over the others.  HIP (through
the C-ABI and through Session) against the oracle: slice ids, scores and tracebacks with ==, the score vector of all slices within
1e-4 (MFMA cosines against the oracle's sums, as test_gpu_wide_query.py::test_long_query_contextual), edge similarities within 2e-6."""

import os

import numpy as np
import pytest

from vectorian_amd import alignment, synth
from vectorian_amd.corpus import Corpus, Document
from vectorian_amd.embedding import StaticEmbedding
from vectorian_amd.session import Session
from vectorian_amd.sim import CosineSim, EmbeddingTokenSim, OptimizedSpanSim

from fake_backend import OracleCorpus
from helpers import assert_same_results

pytestmark = pytest.mark.gpu

EXP5L = ("table", (1 - 2.0 ** (-np.arange(0, 513) / 5)).astype(np.float32))
AFF = ("affine", 0.2, 0.05)
LONG_GAPS = {"linear": (0.1, 0.05), "affine": (AFF, ("affine", 0.1, 0.02)), "exp5": (EXP5L, EXP5L)}   # as test_gpu_wide_query.py
SCALE = int(os.environ.get("VK_SWEEP_SCALE", "1"))

# every block edge: a slice ends one token before, on and one token after every multiple of 64 the kernel can meet
EDGE_LENS = (0, 1, 30, 64, 65, 66, 127, 128, 129, 191, 192, 193, 256, 300, 511, 512)


def mixed_corpus(d, max_len=512, seed=7, n_short=60, V=600):
	"""a contextual corpus with explicit slice lengths: EDGE_LENS (up to max_len) and n_short slices of 1 .. 64 tokens, shuffled"""
	rng = np.random.default_rng(seed)
	lens = np.array([n for n in EDGE_LENS if n <= max_len] + [int(x) for x in rng.integers(1, 65, size=n_short)], dtype=np.int64)
	rng.shuffle(lens)
	off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
	E = synth.make_vocab(V, d)
	ids = synth.zipf_ids(int(off[-1]), V, rng)
	X = np.ascontiguousarray(E[ids] + 0.1 * rng.standard_normal((len(ids), d)).astype(np.float32), dtype=np.float32)
	return dict(X=X, sent_off=off, lens=lens)


def quoting_query(corpus, len_t, seed, into=None):
	"""a query that quotes, with noise, len_t tokens of the corpus from 20 tokens into its longest slice of at most `into` tokens
	(the 300-token slice: tokens 20 .. 20 + len_t cross its block borders at 64, 128, ...), as test_long_query_contextual builds it"""
	rng = np.random.default_rng(seed)
	off, lens = corpus["sent_off"], corpus["lens"]
	s0 = int(np.nonzero(lens == (300 if into is None else into))[0][0])
	toks = (off[s0] + 20 + np.arange(len_t)) % off[-1]
	return s0, corpus["X"][toks] + 0.3 * rng.standard_normal((len_t, corpus["X"].shape[1])).astype(np.float32)


def contextual_handle(hip, corpus, X, precision="bf16"):
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=X.shape[1], n_tokens=X.shape[0], n_sentences=len(corpus["sent_off"]) - 1, precision=precision)
	c.append_vectors(X, normalize=False)
	c.set_sentences(corpus["sent_off"])
	c.finalize()
	return c


class Seen:
	"""what the inputs of a test must have met, so that it cannot pass vacuously"""

	def __init__(self):
		self.long_winner = self.crosses_border = self.short_beside_long = False

	def note(self, lens, got):
		n_tok = lens[np.asarray(got.sentence[:got.n], dtype=np.int64)]
		self.long_winner |= bool((n_tok > 64).any())
		self.short_beside_long |= bool((n_tok > 64).any() and ((n_tok <= 64) & (n_tok > 0)).any())
		for i in range(got.n):
			m = got.mapping[i][got.mapping[i] >= 0]
			if len(m) and int(m.min()) // 64 != int(m.max()) // 64:
				self.crosses_border = True

	def check(self):
		assert self.long_winner and self.crosses_border and self.short_beside_long, vars(self)


def check_contextual(hip, oracle, c, corpus, Xo, Qo, Qh, gap, seen, *, localities=(0, 1, 2), sim=None, q_normalize=False):
	"""one query under every locality against the oracle: the result set, the score vector, the edge similarities, the run without
	tracebacks.  Xo / Qo: what the oracle reads; Qh: what the library is given"""
	off, lens = corpus["sent_off"], corpus["lens"]
	n = len(lens)
	gs, gt = LONG_GAPS[gap]
	# (the boost lifts the slices of at most 64 tokens: winners of both kinds side by side, scored by the two launches)
	boost = (np.random.default_rng(len(Qo)).uniform(0.5, 1.0, size=n) * np.where(lens <= 64, 4.0, 1.0)).astype(np.float32)
	sim = sim or oracle.sim_bf16
	for loc, ms in ((0, 0.0), (1, -1e9), (2, -1e9)):
		if loc not in localities:
			continue
		bst = boost if loc == 2 else None
		kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=9, min_score=ms, boost=bst)
		ref = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=Xo.shape[1], sent_off=off, X=Xo, Q=Qo, want_all_scores=True, n_threads=8, **kw)
		got = c.query(Qh, q_normalize=q_normalize, **kw)
		assert_same_results(got.trimmed(), ref)
		every = c.last_scores()
		np.testing.assert_allclose(every[lens > 0], np.asarray(ref["all_scores"])[lens > 0], atol=1e-4)
		assert np.isneginf(every[lens == 0]).all()
		for i in range(got.n):   # edge similarities of the matched pairs
			s = int(got.sentence[i])
			S = sim(Xo[off[s]:off[s + 1]], Qo)
			for j in np.nonzero(got.mapping[i] >= 0)[0]:
				assert abs(got.edge_sim[i, j] - S[int(got.mapping[i, j]), j]) < 2e-6
		seen.note(lens, got)
		noflow = c.query(Qh, q_normalize=q_normalize, want_flow=False, **kw)
		assert_same_results(noflow.trimmed(), ref, check_mapping=False, score_tol=1e-4, tie_tol=1e-4)


@pytest.mark.parametrize("d,len_t", [(64, 65), (64, 80), (64, 129), (300, 80)])
def test_every_block_edge_contextual(hip, oracle, d, len_t):
	"""slices of 0 .. 512 tokens with every block edge among them, queries of 65 / 80 / 129 tokens that quote a passage inside the
	300-token slice, linear / affine / exp5 gaps, every locality (a boost on one); d = 300: the QFrag fill next to the generic one"""
	corpus = mixed_corpus(d)
	Xb = synth.to_bf16_bits(synth.normalize_rows(corpus["X"]))
	c = contextual_handle(hip, corpus, Xb)
	s0, Q = quoting_query(corpus, len_t, seed=len_t)
	Qb = synth.to_bf16_bits(synth.normalize_rows(Q))
	seen = Seen()
	for gap in ("linear", "affine", "exp5"):
		check_contextual(hip, oracle, c, corpus, Xb, Qb, Qb, gap, seen)
	seen.check()
	c.close()


def test_query_of_512_tokens_linear(hip, oracle):
	corpus = mixed_corpus(64)
	Xb = synth.to_bf16_bits(synth.normalize_rows(corpus["X"]))
	c = contextual_handle(hip, corpus, Xb)
	s0, Q = quoting_query(corpus, 512, seed=512)
	Qb = synth.to_bf16_bits(synth.normalize_rows(Q))
	seen = Seen()
	check_contextual(hip, oracle, c, corpus, Xb, Qb, Qb, "linear", seen)
	seen.check()
	c.close()


def test_query_of_512_tokens_exp5_over_slices_of_up_to_193_tokens(hip, oracle):
	corpus = mixed_corpus(64, max_len=193, n_short=40)
	Xb = synth.to_bf16_bits(synth.normalize_rows(corpus["X"]))
	c = contextual_handle(hip, corpus, Xb)
	s0, Q = quoting_query(corpus, 512, seed=513, into=193)
	Qb = synth.to_bf16_bits(synth.normalize_rows(Q))
	seen = Seen()
	check_contextual(hip, oracle, c, corpus, Xb, Qb, Qb, "exp5", seen)
	seen.check()
	c.close()


def test_f32_precision(hip, oracle):
	"""one linear-gap case of the test above on an fp32 corpus (v_mfma_f32_16x16x4_f32 tiles): the oracle reads the same unrounded rows"""
	corpus = mixed_corpus(64)
	X = oracle.normalize_rows(corpus["X"])
	c = contextual_handle(hip, corpus, X, precision="f32")
	s0, Q = quoting_query(corpus, 80, seed=80)
	Qn = oracle.normalize_rows(Q)
	seen = Seen()
	check_contextual(hip, oracle, c, corpus, X, Qn, Qn, "linear", seen, sim=oracle.sim_f32)
	seen.check()
	c.close()


@pytest.mark.parametrize("len_t,gap", [(80, "linear"), (130, "exp5"), (300, "affine")])
def test_static_layout_tag_weights_a_view_and_listed_slices(hip, oracle, len_t, gap):
	"""the shape of test_long_query_static_with_tag_weights_and_views over slices of up to 200 tokens: tables gathered by token id block
	by block, sim[id(t_j)][j] = 1, a word the vocabulary does not hold, the tag-weighted modifier (the unmodified similarities of the
	edges come from the scratch region), a view beside its owner, and only_slices with short and long slices out of order -- rows of the
	slice table are not slices once a long slice sits in its padded group"""
	corpus = synth.make_static_corpus(300, 1, 50, 400, 96, seed=5)
	lens = np.diff(corpus["sent_off"]).copy()
	lens[[10, 66, 120, 250, 298]] = (200, 70, 130, 65, 128)
	off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
	n_tok = int(off[-1])
	rng = np.random.default_rng(17 + len_t)
	tok_id = synth.zipf_ids(n_tok, 400, rng)
	Eb = synth.to_bf16_bits(synth.normalize_rows(corpus["E"]))
	pos = rng.integers(1, 6, size=n_tok).astype(np.int8)
	c = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=96, n_tokens=n_tok, n_sentences=300, vocab_size=400)
	c.append_vectors(Eb, normalize=False)
	c.set_token_ids(tok_id)
	c.set_token_pos(pos)
	c.set_sentences(off)
	c.finalize()
	q_ids = tok_id[off[10] + 30:off[10] + 30 + len_t].astype(np.int32).copy()   # from inside the 200-token slice on, across its border at 64
	q_ids[5] = -1                                # a word the vocabulary does not hold
	Qb = Eb[np.where(q_ids >= 0, q_ids, 3)]
	gs, gt = LONG_GAPS[gap]
	tw = rng.uniform(0.5, 1.5, size=len_t).astype(np.float32)
	q_pos = rng.integers(1, 6, size=len_t).astype(np.int8)
	v = c.view()
	seen = Seen()
	for loc, ms, tagged in ((0, 0.0, False), (1, -1e9, True), (2, -1e9, True), (0, 0.05, True)):
		okw = dict(tag_weights=tw, q_pos=q_pos, pos_s=pos, pos_mismatch_penalty=0.3, similarity_threshold=0.1) if tagged else {}
		ckw = dict(tag_weights=tw, q_pos=q_pos, pos_mismatch_penalty=0.3, similarity_threshold=0.1) if tagged else {}
		ref = oracle.find(layout=oracle.LAYOUT_STATIC, d=96, sent_off=off, tok_id=tok_id, E=Eb, Q=Qb, q_ids=q_ids, locality=loc,
			gap_s=gs, gap_t=gt, max_matches=7, min_score=ms, n_threads=8, **okw)
		for h in (c, v):
			got = h.query(Qb, q_token_ids=q_ids, q_normalize=False, locality=loc, gap_s=gs, gap_t=gt, max_matches=7, min_score=ms, **ckw)
			assert_same_results(got.trimmed(), ref)
			seen.note(lens, got)
	assert seen.long_winner and seen.crosses_border, vars(seen)
	# only_slices: exactly these slices, in this order, whatever their score; 70, 251 and 299 lie after long slices in the table
	ids = np.array([70, 3, 120, 299, 0, 10, 251, 298, 66], dtype=np.int64)
	got = c.query(Qb, q_token_ids=q_ids, q_normalize=False, locality=0, gap_s=gs, gap_t=gt, only_slices=ids)
	full = oracle.find(layout=oracle.LAYOUT_STATIC, d=96, sent_off=off, tok_id=tok_id, E=Eb, Q=Qb, q_ids=q_ids, locality=0, gap_s=gs, gap_t=gt,
		max_matches=300, min_score=-1.0, n_threads=8)
	by_id = {int(s): i for i, s in enumerate(full["sentence"])}
	assert got.n == len(ids) and (got.sentence[:len(ids)] == ids).all()
	for i, s in enumerate(ids):
		assert got.score[i] == np.float32(full["score"][by_id[int(s)]]) and (got.mapping[i] == full["mapping"][by_id[int(s)]]).all()
	v.close()
	c.close()


def test_what_stays_refused(hip):
	"""whole documents (more than 512 tokens) under a query of more than 64 tokens; the transports and a submatch weight under such a query"""
	rng = np.random.default_rng(2)
	lens = np.array([20, 513, 7, 40], dtype=np.int64)
	off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
	X = rng.standard_normal((int(off[-1]), 32)).astype(np.float32)
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=32, n_tokens=X.shape[0], n_sentences=4)
	c.append_vectors(X, normalize=True)
	c.set_sentences(off)
	c.finalize()
	Q = rng.standard_normal((65, 32)).astype(np.float32)
	with pytest.raises(hip.VkError) as e:
		c.query(Q, max_matches=3)
	assert e.value.status == hip.VK_ERR_UNSUPPORTED
	assert c.query(Q[:64], max_matches=3, min_score=-1e9, locality=1, gap_s=0.1, gap_t=0.1).n == 3
	c.close()
	corpus = mixed_corpus(64)
	c = contextual_handle(hip, corpus, synth.to_bf16_bits(synth.normalize_rows(corpus["X"])))
	assert c.query(Q.repeat(2, axis=1), max_matches=3).n == 3
	for kw in (dict(algorithm=hip.VK_ALG_RWMD), dict(algorithm=hip.VK_ALG_WRD), dict(submatch_weight=0.5)):
		with pytest.raises(hip.VkError) as e:
			c.query(Q.repeat(2, axis=1), max_matches=3, **kw)
		assert e.value.status in (hip.VK_ERR_UNSUPPORTED, hip.VK_ERR_STATE)
	c.close()


def long_sentence_session(seed=3, n_docs=3, sents_per_doc=14, V=400, d=48):
	"""documents whose sentences have 4 .. 40 tokens, but for one of 70 and one of 200 tokens each"""
	rng = np.random.default_rng(seed)
	E = synth.make_vocab(V, d)
	words = [f"w{i}" for i in range(V)]
	docs = []
	for di in range(n_docs):
		n_tok = [int(x) for x in rng.integers(4, 41, size=sents_per_doc)]
		n_tok[3 + di], n_tok[8] = 70, 200
		docs.append(Document([[words[i] for i in synth.zipf_ids(n, V, rng)] for n in n_tok], unique_id=f"doc{di}"))
	emb = StaticEmbedding("toy-48", words, E)
	return Session(Corpus(docs), embeddings=[emb]), emb


@pytest.mark.parametrize("optimizer", [alignment.LocalAlignment(gap=alignment.LinearGapCost(0.1)), alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5))])
@pytest.mark.parametrize("part", [("sentence",), ("sentence", 5, 2)])
def test_through_session(hip, optimizer, part):
	"""a paragraph of 90 tokens as the query over a sentence partition and over windows of five sentences: Index.find, the hook for
	every slice and find_many against the oracle-backed double"""
	from vectorian_amd.index import AllSlices
	session, emb = long_sentence_session()
	sim = OptimizedSpanSim(EmbeddingTokenSim(emb, CosineSim()), optimizer)
	gpu = session.partition(*part).index(sim)
	cpu = session.partition(*part).index(sim, corpus_factory=OracleCorpus)
	assert gpu.n_slices == cpu.n_slices
	doc = session.documents[1]
	st = doc.spans["sentence"]["start"][8]
	paragraphs = [" ".join(doc.tokens[st + 40:st + 130]), " ".join(doc.tokens[st - 30:st + 60]), " ".join(session.documents[2].tokens[5:95])]
	for text in paragraphs[:2]:
		a = gpu.find(text, n=5, min_score=-100.0)
		b = cpu.find(text, n=5, min_score=-100.0)
		assert len(a) == len(b) == 5
		assert [(m.doc_index, m.slice_id) for m in a] == [(m.doc_index, m.slice_id) for m in b]
		assert [m.score for m in a] == [m.score for m in b]
		for x, y in zip(a, b):
			assert (x.flow["target"] == y.flow["target"]).all()
			assert (x.flow["dist"] == y.flow["dist"]).all()
			assert x.to_json() == y.to_json()
		assert a[0].doc_index == 1 and max(m._len_s for m in a) > 64
	calls = {"gpu": [], "cpu": []}
	for name, index in (("gpu", gpu), ("cpu", cpu)):
		index.find(paragraphs[0], n=3, debug=AllSlices(lambda n_, d_, got=calls[name]: got.append((n_, d_)), chunk=16))
	assert len(calls["gpu"]) == len(calls["cpu"]) == gpu.n_slices
	for (na, a), (nb, b) in zip(calls["gpu"], calls["cpu"]):
		assert na == nb == "alignment" and a["slice"] == b["slice"] and a["score"] == b["score"]
		assert (a["flow"]["target"] == b["flow"]["target"]).all() and (a["flow"]["dist"] == b["flow"]["dist"]).all()
	many = gpu.find_many(paragraphs, n=5)
	for text, res in zip(paragraphs, many):
		one = gpu.find(text, n=5)
		assert [(m.doc_index, m.slice_id, m.score) for m in res] == [(m.doc_index, m.slice_id, m.score) for m in one]
		assert all((x.flow["target"] == y.flow["target"]).all() for x, y in zip(res, one))
	gpu.close()
	cpu.close()


def sweep_case(seed):
	"""the draw of one seed of the sweep: (corpus, layout, len_t, gap, locality, min_score)"""
	rng = np.random.default_rng(1000 + seed)
	n = int(rng.integers(40, 90))
	lens = rng.integers(0, 65, size=n)
	long_at = rng.random(n) < 0.1
	lens[long_at] = rng.integers(65, 513, size=int(long_at.sum()))
	if not long_at.any():
		lens[int(rng.integers(0, n))] = int(rng.integers(65, 513))
	off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
	static = bool(rng.integers(0, 2))
	d = int(rng.choice([48, 96, 300]))
	V = 300
	E = synth.make_vocab(V, d, seed=seed + 1)
	ids = synth.zipf_ids(int(off[-1]), V, rng)
	len_t = int(rng.integers(65, 201))
	gap = str(rng.choice(["linear", "affine", "exp5"]))
	if gap == "exp5":   # the oracle's general-gap solver is O(n m (n + m)) per slice: keep the case in seconds
		len_t = min(len_t, 120)
	loc = int(rng.integers(0, 3))
	ms = float(rng.choice([0.0, 0.05, -1e9])) if loc == 0 else -1e9
	s0 = int(np.argmax(lens))
	at = off[s0] + int(rng.integers(0, max(1, lens[s0] - 64)))
	q_tok = (at + np.arange(len_t)) % off[-1]
	return dict(lens=lens, off=off, static=static, d=d, V=V, E=E, ids=ids, len_t=len_t, gap=gap, loc=loc, ms=ms, q_tok=q_tok, rng=rng)


@pytest.mark.parametrize("seed", range(24 * SCALE))
def test_random_sweep(hip, oracle, seed):
	"""len_t 65 .. 200, a tenth of the slices of 65 .. 512 tokens, the gap family, the locality, the layout and min_score drawn per
	seed; ids, scores and mappings == the oracle's, the score vector within 1e-4"""
	k = sweep_case(seed)
	off, lens, d, len_t, rng = k["off"], k["lens"], k["d"], k["len_t"], k["rng"]
	gs, gt = LONG_GAPS[k["gap"]]
	kw = dict(locality=k["loc"], gap_s=gs, gap_t=gt, max_matches=8, min_score=k["ms"])
	if k["static"]:
		Eb = synth.to_bf16_bits(synth.normalize_rows(k["E"]))
		c = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=d, n_tokens=len(k["ids"]), n_sentences=len(lens), vocab_size=k["V"])
		c.append_vectors(Eb, normalize=False)
		c.set_token_ids(k["ids"])
		c.set_sentences(off)
		c.finalize()
		q_ids = k["ids"][k["q_tok"]].astype(np.int32)
		Qb = Eb[q_ids]
		ref = oracle.find(layout=oracle.LAYOUT_STATIC, d=d, sent_off=off, tok_id=k["ids"], E=Eb, Q=Qb, q_ids=q_ids, want_all_scores=True, n_threads=8, **kw)
		got = c.query(Qb, q_token_ids=q_ids, q_normalize=False, **kw)
	else:
		X = k["E"][k["ids"]] + 0.1 * rng.standard_normal((len(k["ids"]), d)).astype(np.float32)
		Xb = synth.to_bf16_bits(synth.normalize_rows(X))
		c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=Xb.shape[0], n_sentences=len(lens))
		c.append_vectors(Xb, normalize=False)
		c.set_sentences(off)
		c.finalize()
		Q = X[k["q_tok"]] + 0.3 * rng.standard_normal((len_t, d)).astype(np.float32)
		Qb = synth.to_bf16_bits(synth.normalize_rows(Q))
		ref = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=d, sent_off=off, X=Xb, Q=Qb, want_all_scores=True, n_threads=8, **kw)
		got = c.query(Qb, q_normalize=False, **kw)
	assert_same_results(got.trimmed(), ref)
	every = c.last_scores()
	np.testing.assert_allclose(every[lens > 0], np.asarray(ref["all_scores"])[lens > 0], atol=1e-4)
	assert np.isneginf(every[lens == 0]).all()
	c.close()
