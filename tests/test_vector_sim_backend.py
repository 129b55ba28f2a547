"""CPU tier: how a vector similarity beside the cosine reaches the backend.  HipBruteForceIndex hands the source to the
corpus it creates -- once, BEFORE the rows are appended, as (kind, float32 argument) -- then the chain, and refuses by name what the
device does not compute.  The C-ABI exports the entry point and refuses a null handle without touching a device."""

import numpy as np
import pytest

from test_host_api import toy_session
from test_sim_ops_backend import _OtherSim, _span
from vector_sim_backend import SourceOracleCorpus, SourceRecordingCorpus
from vectorian_amd import core
from vectorian_amd.corpus import Document
from vectorian_amd.embedding import ContextualEmbedding
from vectorian_amd.session import Session
from vectorian_amd.sim import (CosineSim, DistanceToSimilarity, EmbeddedSpanSim, EuclideanDistance, ImprovedSqrtCosineSim, ModifiedVectorSim,
	PNormDistance, Scale, SpanEmbedding, Threshold, VectorSim)


def test_the_source_reaches_the_corpus_once_before_the_rows():
	session, emb, words, rng = toy_session(n_docs=3, sents_per_doc=20, V=300, d=32)
	part = session.partition("sentence")
	s = 1 / 12
	index = part.index(_span(emb, ModifiedVectorSim(PNormDistance(2), Scale(s), DistanceToSimilarity())), corpus_factory=SourceRecordingCorpus)
	calls = index.corpus.calls
	assert [c[0] for c in calls] == ["set_sim_source", "append_vectors", "set_sim_ops", "finalize"]
	assert calls[0][1] == core.VK_SIMSRC_PNORM and calls[0][2] == np.float32(2) and isinstance(calls[0][2], np.float32)
	assert calls[2][1] == [(core.VK_SIMOP_SCALE, np.float32(s)), (core.VK_SIMOP_ONE_MINUS, np.float32(0))]
	assert index.metric_name == f"toy-300-(1 - (p-norm(2) * {s}))" and index.metric_name.startswith("toy-300-(1 - (p-norm(2) * 0.083")
	# a bare source is legal (its cells are clipped): no chain is set
	bare = part.index(_span(emb, ImprovedSqrtCosineSim()), corpus_factory=SourceRecordingCorpus)
	assert [c[0] for c in bare.corpus.calls] == ["set_sim_source", "append_vectors", "finalize"]
	assert bare.corpus.calls[0][1:] == (core.VK_SIMSRC_SQRT_COSINE, np.float32(0)) and bare.metric_name == "toy-300-improved-sqrt-cosine"
	eu = part.index(_span(emb, ModifiedVectorSim(EuclideanDistance(), Scale(0.1), DistanceToSimilarity(), Threshold(0.2))), corpus_factory=SourceRecordingCorpus)
	assert eu.corpus.calls[0][1:] == (core.VK_SIMSRC_PNORM, np.float32(2)) and eu.metric_name == "toy-300-threshold((1 - (p-norm(2) * 0.1)), 0.2)"
	# the cosine calls neither new method, with a chain or without
	for vsim, names in ((CosineSim(), ["append_vectors", "finalize"]), (ModifiedVectorSim(CosineSim(), Scale(0.5)), ["append_vectors", "set_sim_ops", "finalize"])):
		assert [c[0] for c in part.index(_span(emb, vsim), corpus_factory=SourceRecordingCorpus).corpus.calls] == names


def test_find_under_a_p_norm_on_the_double():
	"""the oracle-backed double under (1 - p-norm(2) * s): the quoted sentence wins with score 1 (every edge is a query word in the
	slice: similarity 1 by the rewrite, and by a distance of exactly 0)"""
	session, emb, words, rng = toy_session(n_docs=3, sents_per_doc=20, V=300, d=32)
	E = emb.encode_tokens(words).unmodified
	s = float(1 / (2 * np.median(np.sqrt(((E[:50, None] - E[None, 50:100]) ** 2).sum(-1)))))
	vsim = ModifiedVectorSim(PNormDistance(2), Scale(s), DistanceToSimilarity())
	index = session.partition("sentence").index(_span(emb, vsim), corpus_factory=SourceOracleCorpus)
	doc = session.documents[1]
	st, en = doc.spans["sentence"]["start"][4], doc.spans["sentence"]["end"][4]
	res = index.find(" ".join(doc.tokens[st:en][:16]), n=5)
	assert res[0].doc_index == 1 and res[0].slice_id == 4 and res[0].score == 1.0
	assert [m.score for m in res] == sorted((m.score for m in res), reverse=True) and 0 < res[4].score < 1
	many = index.find_many([" ".join(doc.tokens[st:en][:16])], n=5)
	assert [(m.doc_index, m.slice_id, m.score) for m in many[0]] == [(m.doc_index, m.slice_id, m.score) for m in res]


class _FuzzyJaccardSim(VectorSim):
	@property
	def name(self):
		return "fuzzy-jaccard"


class _MyNorm(PNormDistance):   # a subclass may compute anything
	pass


def test_what_stays_refused_says_which_case_it_is():
	session, emb, words, rng = toy_session(n_docs=2, sents_per_doc=5, V=100, d=16)
	part = session.partition("sentence")

	def refused(sim, *words_in_message, session_=part):
		with pytest.raises(NotImplementedError) as e:
			session_.index(sim, corpus_factory=SourceRecordingCorpus)
		for w in words_in_message:
			assert w in str(e.value), (w, str(e.value))
	refused(_span(emb, _FuzzyJaccardSim()), "fuzzy-jaccard", "CosineSim", "PNormDistance", "ImprovedSqrtCosineSim")
	refused(_span(emb, ModifiedVectorSim(_FuzzyJaccardSim(), Scale(0.5))), "fuzzy-jaccard", "CosineSim only", "PNormDistance")
	refused(_span(emb, ModifiedVectorSim(_OtherSim(), Scale(0.5))), "CosineSim only", "other")
	refused(_span(emb, _MyNorm(2)), "p-norm(2)", "not other VectorSims")
	refused(_span(emb, ModifiedVectorSim(PNormDistance(0), DistanceToSimilarity())), "p-norm(0)", "finite and > 0")
	refused(_span(emb, PNormDistance(float("inf"))), "p-norm(inf)", "finite and > 0")
	refused(_span(emb, PNormDistance(-1)), "finite and > 0")
	# a contextual embedding
	d = 16
	vecs = np.random.default_rng(0).standard_normal((100, d)).astype(np.float32)
	ctx = ContextualEmbedding("ctx", d, lambda tokens: np.stack([vecs[int(t[1:])] for t in tokens]))
	toks = [["w1", "w2", "w3"], ["w4", "w5"]]
	docs = [Document(toks, contextual_embeddings={"ctx": np.stack([vecs[int(t[1:])] for s in toks for t in s])})]
	csession = Session(docs, embeddings=[ctx])
	refused(_span(ctx, PNormDistance(2)), "p-norm(2)", "static embeddings only", "ctx is contextual", session_=csession)
	refused(_span(ctx, ModifiedVectorSim(ImprovedSqrtCosineSim(), Scale(0.5))), "improved-sqrt-cosine", "static embeddings only", "ctx is contextual", session_=csession)
	# the span index computes the plain cosine
	with pytest.raises(NotImplementedError) as e:
		part.index(EmbeddedSpanSim(SpanEmbedding("mean", 16, lambda texts: np.zeros((len(texts), 16))), PNormDistance(2)), corpus_factory=SourceRecordingCorpus)
	assert "p-norm(2)" in str(e.value) and "CosineSim" in str(e.value)


def test_the_entry_point_is_exported_and_refuses_a_null_handle():
	lib = core.lib()
	assert "vk_corpus_set_sim_source" in core.EXPORTS and hasattr(lib, "vk_corpus_set_sim_source")
	assert lib.vk_corpus_set_sim_source(None, core.VK_SIMSRC_PNORM, 2.0) == core.VK_ERR_INVALID
	assert b"null" in lib.vk_last_error()
	assert lib.vk_corpus_set_sim_source(None, core.VK_SIMSRC_COSINE, 0.0) == core.VK_ERR_INVALID
	assert lib.vk_abi_version() == 12
