"""CPU tier: what HipSpanEncoderIndex asks its backend under a VectorSim that is not the bare CosineSim, against a
recording double of core.Corpus that HAS set_span_sim: the order of the calls (set_span_sim before the first append), the
(kind, float32 arg) payloads of every source and of a six-operator chain, today's calls under the bare cosine, every refusal by
name -- and, on a double WITHOUT the method, the capability refusal that names the similarity."""

import ctypes as C

import numpy as np
import pytest

import pool_cases as pc
from fake_backend import OracleCorpus
from vectorian_amd import core
from vectorian_amd import kernel as K
from vectorian_amd.sim import (AggregatedSpanEmbedding, Bias, CosineSim, DistanceToSimilarity, EmbeddedSpanSim, EuclideanDistance,
	ImprovedSqrtCosineSim, ModifiedVectorSim, PNormDistance, Power, RadialBasis, Scale, SpanEmbedding, Threshold, VectorSim)

NAMES = ("set_span_sim", "append_vectors", "append_pooled", "set_sentences", "finalize", "close")


class Recording(OracleCorpus):
	"""core.Corpus's interface on the oracle, set_span_sim and append_pooled included, with a log of the calls an index makes"""
	log = None

	def set_span_sim(self, source=None, ops=()):
		Recording.log.append(("set_span_sim", source, list(ops)))

	def append_vectors(self, rows, normalize=True):
		if not getattr(self, "_pooling", False):
			Recording.log.append(("append_vectors", np.array(rows), normalize))
		super().append_vectors(rows, normalize=normalize)

	def append_pooled(self, rows, start, end, agg, ids=None, normalize=True, want_pooled=False):
		Recording.log.append(("append_pooled", agg, normalize))
		self._pooling = True
		try:
			self.append_vectors(np.zeros((len(start), self.d), np.float32), normalize=normalize)
		finally:
			self._pooling = False

	def set_sentences(self, off):
		Recording.log.append(("set_sentences", len(off) - 1))
		super().set_sentences(off)

	def finalize(self):
		Recording.log.append(("finalize",))
		super().finalize()

	def close(self):
		Recording.log.append(("close",))
		super().close()


class WithoutTheMethod(OracleCorpus):
	closed = 0

	def close(self):
		WithoutTheMethod.closed += 1
		super().close()


def given_index(sim, factory=Recording, d=12, n_docs=3):
	"""an index over span vectors from the caller"""
	from test_host_api import Document, Session
	docs = [Document([[f"s{i}"] for i in range(10)]) for _ in range(n_docs)]
	session = Session(docs, embeddings=[])
	vectors = np.random.default_rng(3).standard_normal((10 * n_docs, d)).astype(np.float32)
	emb = SpanEmbedding("enc", d, lambda texts: np.ones((len(texts), d), np.float32))
	Recording.log = []
	return session.partition("sentence").index(EmbeddedSpanSim(emb, sim), vectors=vectors, corpus_factory=factory), vectors


SOURCES = [
	(PNormDistance(2), (core.VK_SIMSRC_PNORM, np.float32(2))),
	(PNormDistance(1), (core.VK_SIMSRC_PNORM, np.float32(1))),
	(PNormDistance(0.5), (core.VK_SIMSRC_PNORM, np.float32(0.5))),
	(PNormDistance(3), (core.VK_SIMSRC_PNORM, np.float32(3))),
	(EuclideanDistance(), (core.VK_SIMSRC_PNORM, np.float32(2))),
	(ImprovedSqrtCosineSim(), (core.VK_SIMSRC_SQRT_COSINE, np.float32(0))),
]


@pytest.mark.parametrize("sim,payload", SOURCES, ids=lambda x: getattr(x, "name", None))
def test_a_bare_source_is_set_before_the_first_append(sim, payload):
	index, vectors = given_index(sim)
	try:
		assert [e[0] for e in Recording.log] == ["set_span_sim", "append_vectors", "set_sentences", "finalize"]
		_, source, ops = Recording.log[0]
		assert source == payload and isinstance(source[0], int) and isinstance(source[1], np.float32) and ops == []
		assert np.array_equal(Recording.log[1][1], vectors) and Recording.log[1][2] is True
	finally:
		index.close()


def test_a_six_operator_chain_and_its_source():
	chain = [Bias(1), Scale(0.5), Threshold(0.3), DistanceToSimilarity(), Power(2.5), RadialBasis(1.5)]
	for src, payload in [(CosineSim(), None)] + SOURCES[:1] + SOURCES[-1:]:
		index, _ = given_index(ModifiedVectorSim(src, *chain))
		try:
			assert [e[0] for e in Recording.log] == ["set_span_sim", "append_vectors", "set_sentences", "finalize"]
			_, source, ops = Recording.log[0]
			assert source == payload
			assert [k for k, _ in ops] == [core.VK_SIMOP_BIAS, core.VK_SIMOP_SCALE, core.VK_SIMOP_THRESHOLD, core.VK_SIMOP_ONE_MINUS, core.VK_SIMOP_POWER,
				core.VK_SIMOP_RADIAL_BASIS]
			assert all(isinstance(k, int) and isinstance(a, np.float32) for k, a in ops)
			assert [a for _, a in ops] == [np.float32(x) for x in (1, 0.5, 0.3, 0, 2.5, 1.5)]
		finally:
			index.close()
	# eight operators are the most
	index, _ = given_index(ModifiedVectorSim(CosineSim(), *([Bias(0.5), Scale(0.5)] * 4)))
	assert len(Recording.log[0][2]) == 8
	index.close()


@pytest.mark.parametrize("sim", [None, CosineSim(), ModifiedVectorSim(CosineSim())], ids=["default", "cosine", "empty-chain"])
def test_the_bare_cosine_makes_todays_calls(sim):
	index, _ = given_index(sim)
	assert [e[0] for e in Recording.log] == ["append_vectors", "set_sentences", "finalize"]
	index.close()
	assert Recording.log[-1] == ("close",)


@pytest.mark.parametrize("embedding,appends", [("static", 1), ("contextual", 40)])
def test_pooled_spans_under_a_distance(embedding, appends):
	session, embeddings, texts = pc.toy_session()
	emb = AggregatedSpanEmbedding(embeddings[embedding], np.mean)
	sim = ModifiedVectorSim(PNormDistance(2), Scale(0.25), DistanceToSimilarity())
	Recording.log = []
	index = session.partition("sentence").index(emb.to_sentence_sim(sim), corpus_factory=Recording)
	try:
		assert [e[0] for e in Recording.log] == ["set_span_sim"] + ["append_pooled"] * appends + ["set_sentences", "finalize"]
		assert Recording.log[0][1] == (core.VK_SIMSRC_PNORM, np.float32(2))
		assert Recording.log[0][2] == [(core.VK_SIMOP_SCALE, np.float32(0.25)), (core.VK_SIMOP_ONE_MINUS, np.float32(0))]
		assert index.sim.vector_sim is sim and emb.to_sentence_sim(sim).name == "EmbeddedSpanSim"
	finally:
		index.close()


class _FuzzyJaccardSim(VectorSim):
	@property
	def name(self):
		return "fuzzy-jaccard"


class _DirectionalDistance(VectorSim):
	@property
	def name(self):
		return "directional"


class _MyNorm(PNormDistance):
	pass


class _MySqrt(ImprovedSqrtCosineSim):
	pass


class _Mine(K.UnaryOperator):
	def kernel(self, data):
		data *= 2


@pytest.mark.parametrize("sim,words", [
	(_FuzzyJaccardSim(), ("fuzzy-jaccard", "CosineSim", "PNormDistance", "ImprovedSqrtCosineSim", "not other VectorSims")),
	(_DirectionalDistance(), ("directional", "not other VectorSims")),
	(ModifiedVectorSim(_FuzzyJaccardSim(), Scale(0.5)), ("fuzzy-jaccard", "modifies CosineSim", "PNormDistance")),
	(ModifiedVectorSim(_DirectionalDistance(), DistanceToSimilarity()), ("directional", "modifies CosineSim")),
	(_MyNorm(2), ("p-norm(2)", "not other VectorSims")),
	(ModifiedVectorSim(_MySqrt(), Scale(0.5)), ("improved-sqrt-cosine", "modifies CosineSim")),
	(PNormDistance(0), ("p-norm(0)", "finite and > 0")),
	(PNormDistance(float("inf")), ("p-norm(inf)", "finite and > 0")),
	(PNormDistance(float("nan")), ("finite and > 0",)),
	(ModifiedVectorSim(PNormDistance(-1), DistanceToSimilarity()), ("finite and > 0",)),
	(ModifiedVectorSim(ModifiedVectorSim(CosineSim(), Bias(1)), Scale(0.5)), ("nested ModifiedVectorSim",)),
	(ModifiedVectorSim(CosineSim(), *([Bias(0.1)] * 9)), ("9 operators", "at most 8")),
	(ModifiedVectorSim(CosineSim(), _Mine()), ("_Mine", "vectorian_amd.kernel")),
])
def test_every_refusal_by_name(sim, words):
	with pytest.raises(NotImplementedError) as e:
		given_index(sim)
	for w in words:
		assert w in str(e.value), (w, str(e.value))
	assert "contextual" not in str(e.value)       # a span vector is nobody's token: no "static embeddings only"
	assert Recording.log == []                      # refused before a corpus is made


@pytest.mark.parametrize("sim", [PNormDistance(2), ImprovedSqrtCosineSim(), ModifiedVectorSim(CosineSim(), Bias(1)),
	ModifiedVectorSim(PNormDistance(1), Scale(0.5), DistanceToSimilarity())], ids=lambda s: s.name)
def test_a_backend_without_the_method_refuses_by_capability(sim):
	WithoutTheMethod.closed = 0
	with pytest.raises(NotImplementedError) as e:
		given_index(sim, factory=WithoutTheMethod)
	assert sim.name in str(e.value) and "CosineSim" in str(e.value)
	assert WithoutTheMethod.closed == 1           # the corpus it had just made is closed
	# ... and the bare cosine still runs on it
	index, _ = given_index(CosineSim(), factory=WithoutTheMethod)
	index.close()


def test_a_type_that_is_no_vector_sim():
	with pytest.raises(TypeError):
		EmbeddedSpanSim(SpanEmbedding("enc", 4, lambda t: np.zeros((len(t), 4))), "cosine")


def test_the_entry_point_is_exported_and_validates_without_a_device():
	lib = core.lib()
	assert "vk_corpus_set_span_sim" in core.EXPORTS and hasattr(lib, "vk_corpus_set_span_sim") and hasattr(core.Corpus, "set_span_sim")
	kinds, args = np.zeros(2, np.int32), np.ones(2, np.float32)
	ptr = lambda a: a.ctypes.data_as(C.c_void_p)
	assert lib.vk_corpus_set_span_sim(None, core.VK_SIMSRC_PNORM, 2.0, ptr(kinds), ptr(args), 2) == core.VK_ERR_INVALID
	assert b"null" in lib.vk_last_error()
	assert lib.vk_abi_version() == 12
