"""CPU tier: how a ModifiedVectorSim over a ContextualEmbedding reaches the backend.  HipBruteForceIndex hands the chain
to the corpus it creates through `set_contextual_sim_ops` -- once, after the vectors are appended and before finalize, as (kind,
float32 argument) pairs -- if the backend has that method, and refuses by name what the device does not compute.  The C-ABI exports
the entry point and refuses a null handle without touching a device."""

import ctypes as C

import numpy as np
import pytest

from sim_ops_backend import RecordingCorpus
from vectorian_amd import alignment, core
from vectorian_amd import kernel as K
from vectorian_amd.corpus import Document
from vectorian_amd.embedding import ContextualEmbedding, StaticEmbedding
from vectorian_amd.modifier import MaximumTokenSimilarity, UnaryTokenSimilarityModifier
from vectorian_amd.session import Session
from vectorian_amd.sim import (Bias, CosineSim, DistanceToSimilarity, EmbeddingTokenSim, ImprovedSqrtCosineSim, ModifiedVectorSim, OptimizedSpanSim,
	PNormDistance, Power, RadialBasis, Scale, Threshold)


class ContextualRecordingCorpus(RecordingCorpus):
	"""the recording double with the capability: notes the appends too, so that the order of the calls can be read"""

	def append_vectors(self, rows, normalize=True):
		self.calls.append(("append_vectors", len(rows)))
		super().append_vectors(rows, normalize=normalize)

	def set_contextual_sim_ops(self, ops):
		self.calls.append(("set_contextual_sim_ops", [(k, a) for k, a in ops]))


def _span(emb, vsim):
	return OptimizedSpanSim(EmbeddingTokenSim(emb, vsim), alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5)))


@pytest.fixture(scope="module")
def ctx_session():
	d = 16
	vecs = np.random.default_rng(0).standard_normal((100, d)).astype(np.float32)
	ctx = ContextualEmbedding("ctx", d, lambda tokens: np.stack([vecs[int(t[1:])] for t in tokens]))
	static = StaticEmbedding("st", [f"w{i}" for i in range(100)], vecs)
	docs = []
	for toks in ([["w1", "w2", "w3"], ["w4", "w5"]], [["w6", "w7"], ["w8", "w9", "w10", "w11"]]):
		docs.append(Document(toks, contextual_embeddings={"ctx": np.stack([vecs[int(t[1:])] for s in toks for t in s])}))
	return Session(docs, embeddings=[static, ctx]), ctx, static


def test_the_chain_reaches_the_corpus_once_after_the_appends_and_before_finalize(ctx_session):
	session, ctx, _ = ctx_session
	vsim = ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5), Threshold(0.3), DistanceToSimilarity(), Power(2.5), RadialBasis(1.5))
	index = session.partition("sentence").index(_span(ctx, vsim), corpus_factory=ContextualRecordingCorpus)
	names = [c[0] for c in index.corpus.calls]
	assert names == ["append_vectors", "append_vectors", "set_contextual_sim_ops", "finalize"]   # one append per document
	ops = index.corpus.calls[2][1]
	assert [k for k, _ in ops] == [core.VK_SIMOP_BIAS, core.VK_SIMOP_SCALE, core.VK_SIMOP_THRESHOLD, core.VK_SIMOP_ONE_MINUS, core.VK_SIMOP_POWER,
		core.VK_SIMOP_RADIAL_BASIS]
	assert all(isinstance(a, np.float32) for _, a in ops)
	assert [a for _, a in ops] == [np.float32(x) for x in (1, 0.5, 0.3, 0, 2.5, 1.5)]
	assert index.metric_name == "ctx-radialbasis(((1 - threshold(((cosine + 1) * 0.5), 0.3)) ** 2.5), 1.5)"
	# the plain cosine sets nothing
	plain = session.partition("sentence").index(_span(ctx, CosineSim()), corpus_factory=ContextualRecordingCorpus)
	assert [c[0] for c in plain.corpus.calls] == ["append_vectors", "append_vectors", "finalize"] and plain.metric_name == "ctx-cosine"
	# eight operators are the most
	eight = ModifiedVectorSim(CosineSim(), *([Bias(0.5), Scale(0.5)] * 4))
	calls = session.partition("sentence").index(_span(ctx, eight), corpus_factory=ContextualRecordingCorpus).corpus.calls
	assert len([c for c in calls if c[0] == "set_contextual_sim_ops"][0][1]) == 8


def test_a_backend_without_the_method_refuses_as_before(ctx_session):
	session, ctx, _ = ctx_session
	with pytest.raises(NotImplementedError) as e:
		session.partition("sentence").index(_span(ctx, ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5))), corpus_factory=RecordingCorpus)
	assert "static embeddings only" in str(e.value) and "ctx is contextual" in str(e.value) and "((cosine + 1) * 0.5)" in str(e.value)


def test_what_stays_refused_over_contextual_embeddings(ctx_session):
	session, ctx, static = ctx_session
	part = session.partition("sentence")

	def refused(sim, *words):
		with pytest.raises(NotImplementedError) as e:
			part.index(sim, corpus_factory=ContextualRecordingCorpus)
		for w in words:
			assert w in str(e.value), (w, str(e.value))
	refused(_span(ctx, PNormDistance(2)), "p-norm(2)", "static embeddings only", "ctx is contextual")
	refused(_span(ctx, ModifiedVectorSim(ImprovedSqrtCosineSim(), Scale(0.5))), "improved-sqrt-cosine", "static embeddings only", "ctx is contextual")
	refused(_span(ctx, ModifiedVectorSim(CosineSim(), *([Bias(0.1)] * 9))), "9 operators", "at most 8")
	refused(_span(ctx, ModifiedVectorSim(ModifiedVectorSim(CosineSim(), Bias(1)), Scale(0.5))), "nested ModifiedVectorSim")

	class Mine(K.UnaryOperator):
		def kernel(self, data):
			data *= 2
	refused(_span(ctx, ModifiedVectorSim(CosineSim(), Mine())), "Mine", "vectorian_amd.kernel")
	opt = alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5))
	both = MaximumTokenSimilarity([EmbeddingTokenSim(static, CosineSim()), EmbeddingTokenSim(ctx, ModifiedVectorSim(CosineSim(), Bias(1)))])
	refused(OptimizedSpanSim(both, opt), "combinators run over static embeddings only", "ctx is contextual")
	unary = UnaryTokenSimilarityModifier(EmbeddingTokenSim(ctx, CosineSim()), [Bias(1)])
	refused(OptimizedSpanSim(unary, opt), "UnaryTokenSimilarityModifier", "ModifiedVectorSim")


def test_the_entry_point_is_exported_and_refuses_a_null_handle():
	lib = core.lib()
	assert "vk_corpus_set_contextual_sim_ops" in core.EXPORTS and hasattr(lib, "vk_corpus_set_contextual_sim_ops")
	assert hasattr(core.Corpus, "set_contextual_sim_ops")
	kinds, args = np.zeros(2, np.int32), np.ones(2, np.float32)
	assert lib.vk_corpus_set_contextual_sim_ops(None, kinds.ctypes.data_as(C.c_void_p), args.ctypes.data_as(C.c_void_p), 2) == core.VK_ERR_INVALID
	assert b"null" in lib.vk_last_error()
	assert lib.vk_corpus_set_contextual_sim_ops(None, None, None, 0) == core.VK_ERR_INVALID
	assert core.VK_MAX_SIM_OPS == 8 and lib.vk_abi_version() == 12
