"""CPU tier: how a ModifiedVectorSim reaches the backend.  HipBruteForceIndex hands the chain of operators to the corpus it creates --
once, before finalize, as (kind, float32 argument) pairs -- and refuses, by name, what the device does not compute.  The C-ABI exports
the entry point and refuses a null handle without touching a device."""

import ctypes as C

import numpy as np
import pytest

import sim_ops_cases as sc
from sim_ops_backend import ChainOracleCorpus, RecordingCorpus
from test_host_api import toy_session
from vectorian_amd import alignment, core
from vectorian_amd import kernel as K
from vectorian_amd.embedding import ContextualEmbedding
from vectorian_amd.corpus import Document
from vectorian_amd.session import Session
from vectorian_amd.sim import (Bias, CosineSim, DistanceToSimilarity, EmbeddedSpanSim, EmbeddingTokenSim, ModifiedVectorSim, OptimizedSpanSim,
	Power, RadialBasis, Scale, SpanEmbedding, Threshold, TokenSim, VectorSim)


def _span(emb, vsim):
	return OptimizedSpanSim(EmbeddingTokenSim(emb, vsim), alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5)))


def test_the_chain_reaches_the_corpus_once_before_finalize():
	session, emb, words, rng = toy_session(n_docs=3, sents_per_doc=20, V=300, d=32)
	vsim = ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5), Threshold(0.3), DistanceToSimilarity(), Power(2.5), RadialBasis(1.5))
	index = session.partition("sentence").index(_span(emb, vsim), corpus_factory=RecordingCorpus)
	calls = index.corpus.calls
	assert [c[0] for c in calls] == ["set_sim_ops", "finalize"]
	ops = calls[0][1]
	assert [k for k, _ in ops] == [core.VK_SIMOP_BIAS, core.VK_SIMOP_SCALE, core.VK_SIMOP_THRESHOLD, core.VK_SIMOP_ONE_MINUS, core.VK_SIMOP_POWER,
		core.VK_SIMOP_RADIAL_BASIS]
	assert all(isinstance(a, np.float32) for _, a in ops)
	assert [a for _, a in ops] == [np.float32(x) for x in (1, 0.5, 0.3, 0, 2.5, 1.5)]
	assert index.metric_name == "toy-300-radialbasis(((1 - threshold(((cosine + 1) * 0.5), 0.3)) ** 2.5), 1.5)"
	# the plain cosine sets nothing
	plain = session.partition("sentence").index(_span(emb, CosineSim()), corpus_factory=RecordingCorpus)
	assert [c[0] for c in plain.corpus.calls] == ["finalize"] and plain.metric_name == "toy-300-cosine"
	# eight operators are the most
	eight = ModifiedVectorSim(CosineSim(), *([Bias(0.5), Scale(0.5)] * 4))
	assert len(session.index(_span(emb, eight), corpus_factory=RecordingCorpus).corpus.calls[0][1]) == 8


def test_find_under_a_chain_on_the_double_and_its_filtered_corpus():
	"""the oracle-backed double under (a): negative cosines count, a query word in a slice is an edge of similarity 1"""
	session, emb, words, rng = toy_session(n_docs=3, sents_per_doc=20, V=300, d=32)
	vsim = ModifiedVectorSim(CosineSim(), *sc.chain("a"))
	index = session.partition("sentence").index(_span(emb, vsim), corpus_factory=ChainOracleCorpus)
	doc = session.documents[1]
	st = doc.spans["sentence"]["start"][4]
	res = index.find(" ".join(doc.tokens[st:st + 5]), n=5)
	assert res[0].doc_index == 1 and res[0].slice_id == 4 and abs(res[0].score - 1.0) < 1e-6
	assert [m.score for m in res] == sorted((m.score for m in res), reverse=True) and res[4].score > 0.55   # (cos + 1) / 2: about 0.5 for unrelated words
	many = index.find_many([" ".join(doc.tokens[st:st + 5])], n=5)
	assert [(m.doc_index, m.slice_id, m.score) for m in many[0]] == [(m.doc_index, m.slice_id, m.score) for m in res]


class _OtherSim(VectorSim):
	@property
	def name(self):
		return "other"


def test_what_stays_refused_says_which_case_it_is():
	session, emb, words, rng = toy_session(n_docs=2, sents_per_doc=5, V=100, d=16)
	part = session.partition("sentence")

	def refused(sim, *words_in_message):
		with pytest.raises(NotImplementedError) as e:
			part.index(sim, corpus_factory=RecordingCorpus)
		for w in words_in_message:
			assert w in str(e.value), (w, str(e.value))
	refused(_span(emb, ModifiedVectorSim(CosineSim(), *([Bias(0.1)] * 9))), "9 operators", "at most 8")
	refused(_span(emb, ModifiedVectorSim(_OtherSim(), Bias(1))), "CosineSim only", "other")
	refused(_span(emb, ModifiedVectorSim(ModifiedVectorSim(CosineSim(), Bias(1)), Scale(0.5))), "nested ModifiedVectorSim")
	refused(_span(emb, _OtherSim()), "other", "CosineSim")

	class Modifier(TokenSim):   # the reference's TokenSimilarityModifier family: Unary.., Mixed.., Maximum.. / Minimum..
		is_modifier = True
	refused(OptimizedSpanSim(Modifier()), "token similarity modifiers", "ModifiedVectorSim")

	class Mine(K.UnaryOperator):
		def kernel(self, data):
			data *= 2
	refused(_span(emb, ModifiedVectorSim(CosineSim(), Mine())), "Mine", "vectorian_amd.kernel")
	# a contextual embedding under a chain
	d = 16
	vecs = np.random.default_rng(0).standard_normal((100, d)).astype(np.float32)
	ctx = ContextualEmbedding("ctx", d, lambda tokens: np.stack([vecs[int(t[1:])] for t in tokens]))
	toks = [["w1", "w2", "w3"], ["w4", "w5"]]
	docs = [Document(toks, contextual_embeddings={"ctx": np.stack([vecs[int(t[1:])] for s in toks for t in s])})]
	csession = Session(docs, embeddings=[ctx])
	with pytest.raises(NotImplementedError) as e:
		csession.index(_span(ctx, ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5))), corpus_factory=RecordingCorpus)
	assert "static embeddings only" in str(e.value) and "ctx is contextual" in str(e.value)
	# the span index computes the plain cosine
	with pytest.raises(NotImplementedError) as e:
		part.index(EmbeddedSpanSim(SpanEmbedding("mean", 16, lambda texts: np.zeros((len(texts), 16))), ModifiedVectorSim(CosineSim(), Bias(1))), corpus_factory=RecordingCorpus)
	assert "(cosine + 1)" in str(e.value) and "CosineSim" in str(e.value)


def test_the_entry_point_is_exported_and_refuses_a_null_handle():
	lib = core.lib()
	assert "vk_corpus_set_sim_ops" in core.EXPORTS and hasattr(lib, "vk_corpus_set_sim_ops")
	kinds, args = np.zeros(2, np.int32), np.ones(2, np.float32)
	assert lib.vk_corpus_set_sim_ops(None, kinds.ctypes.data_as(C.c_void_p), args.ctypes.data_as(C.c_void_p), 2) == core.VK_ERR_INVALID
	assert b"null" in lib.vk_last_error()
	assert lib.vk_corpus_set_sim_ops(None, None, None, 0) == core.VK_ERR_INVALID
	assert core.VK_MAX_SIM_OPS == 8 and lib.vk_abi_version() == 12
