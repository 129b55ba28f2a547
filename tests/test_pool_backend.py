"""CPU tier: AggregatedSpanEmbedding and the span index built from it, against a recording double of core.Corpus on the
oracle: which append_pooled calls HipSpanEncoderIndex makes -- one per document over a contextual embedding, one over a static one,
the slices HipBruteForceIndex enumerates for sentences, windows and documents -- the names, the refusals, and what encode() makes of
a query."""

import numpy as np
import pytest

import pool_cases as pc
from fake_backend import OracleCorpus
from vectorian_amd import core
from vectorian_amd.sim import (AggregatedSpanEmbedding, CosineSim, EmbeddedSpanSim, EmbeddingTokenSim, OptimizedSpanSim, PNormDistance,
	SpanEmbedding)

PARTITIONS = [("sentence", 1, None), ("sentence", 3, 2), ("document", 1, None)]


class Recording(OracleCorpus):
	"""core.Corpus's interface on the oracle, append_pooled included: numpy's aggregate of every span, appended as rows"""
	log = None

	def append_vectors(self, rows, normalize=True):
		if not getattr(self, "_pooling", False):
			Recording.log.append(("append_vectors", np.array(rows), normalize))
		super().append_vectors(rows, normalize=normalize)

	def append_pooled(self, rows, start, end, agg, ids=None, normalize=True, want_pooled=False):
		rows, start, end = np.asarray(rows), np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
		Recording.log.append(("append_pooled", rows, start, end, agg, None if ids is None else np.asarray(ids), normalize))
		assert core.pool_code(agg) in (core.VK_POOL_MEAN, core.VK_POOL_MIN, core.VK_POOL_MAX)
		pooled = np.full((len(start), self.d), np.nan, np.float32)
		for i, (a, b) in enumerate(zip(start, end)):
			v = rows[a:b] if ids is None else rows[np.asarray(ids)[a:b]]
			if len(v):
				pooled[i] = agg(v, axis=0)
		self._pooling = True
		try:
			self.append_vectors(np.nan_to_num(pooled, nan=0.0), normalize=normalize)
		finally:
			self._pooling = False
		return pooled if want_pooled else None


def brute_force_slices(session, part, embedding):
	"""the slices of HipBruteForceIndex over the same partition: global token ranges, document and slice id of each"""
	index = part.index(OptimizedSpanSim(EmbeddingTokenSim(embedding, CosineSim())), corpus_factory=OracleCorpus)
	try:
		return index._slice_start, index._slice_end, list(index._slice_doc), list(index._slice_id)
	finally:
		index.close()


@pytest.mark.parametrize("partition", PARTITIONS)
def test_a_static_embedding_is_pooled_in_one_call(partition):
	session, embeddings, _ = pc.toy_session()
	part = session.partition(*partition)
	emb = AggregatedSpanEmbedding(embeddings["static"], np.max)
	Recording.log = []
	index = part.index(emb.to_sentence_sim(), corpus_factory=Recording)
	try:
		assert [entry[0] for entry in Recording.log] == ["append_pooled"]
		_, rows, start, end, agg, ids, normalize = Recording.log[0]
		assert agg is np.max and normalize is True
		# the vocabulary's unmodified rows ("unseen": a zero row) and the documents' token ids
		assert np.array_equal(rows, embeddings["static"].encode_tokens(session.vocab.tokens).unmodified)
		assert not rows[session.vocab.token_to_id("unseen")].any()
		assert np.array_equal(ids, np.concatenate([session.doc_token_ids(i) for i in range(len(session.documents))]))
		s, e, docs, sids = brute_force_slices(session, part, embeddings["static"])
		assert np.array_equal(start, s) and np.array_equal(end, e)
		assert list(index._slice_doc) == docs and list(index._slice_id) == sids
		assert index._corpus.n_sentences == len(s) and index._corpus.layout == core.VK_LAYOUT_CONTEXTUAL
	finally:
		index.close()


@pytest.mark.parametrize("partition", PARTITIONS)
def test_a_contextual_embedding_is_pooled_document_by_document(partition):
	session, embeddings, _ = pc.toy_session()
	part = session.partition(*partition)
	emb = AggregatedSpanEmbedding(embeddings["contextual"], np.mean)
	Recording.log = []
	index = part.index(emb.to_sentence_sim(), corpus_factory=Recording)
	try:
		assert [entry[0] for entry in Recording.log] == ["append_pooled"] * len(session.documents)
		s, e, docs, _ = brute_force_slices(session, part, embeddings["contextual"])
		base, at = 0, 0
		for di, (doc, (_, rows, start, end, agg, ids, normalize)) in enumerate(zip(session.documents, Recording.log)):
			assert agg is np.mean and ids is None and normalize is True
			assert rows is doc.contextual_vectors("toy-contextual") or np.array_equal(rows, doc.contextual_vectors("toy-contextual"))
			n = docs.count(di)
			assert np.array_equal(start + base, s[at:at + n]) and np.array_equal(end + base, e[at:at + n])   # the document's own tokens
			assert [(a, b) for _, a, b in pc.window_ranges(doc, part)] == list(zip(start.tolist(), end.tolist()))
			base, at = base + doc.n_tokens, at + n
		assert at == len(s)
	finally:
		index.close()


@pytest.mark.parametrize("embedding", ["static", "contextual"])
def test_the_index_finds_what_the_reference_loop_finds(embedding):
	"""through the double: a pooled index and one given the reference's loop as vectors= return the same matches"""
	session, embeddings, texts = pc.toy_session()
	part = session.partition("sentence", 3, 2)
	key = lambda result: [(session.documents.index(m.prepared_doc), m.slice_id, m.score) for m in result]
	for agg in (np.mean, np.min, np.max):
		emb = AggregatedSpanEmbedding(embeddings[embedding], agg)
		Recording.log = []
		pooled = part.index(emb.to_sentence_sim(), corpus_factory=Recording)
		given = part.index(emb.to_sentence_sim(), vectors=pc.reference_span_vectors(session, part, emb), corpus_factory=Recording)
		# given vectors=, the constructor behaves as it always did, whatever the embedding
		assert Recording.log[-1][0] == "append_vectors" and Recording.log[-1][2] is True
		for text in texts[:3]:
			a, b = pooled.find(text, n=4), given.find(text, n=4)
			assert len(a) >= 1 and key(a) == key(b)
		assert [key(r) for r in pooled.find_many(texts, n=4)] == [key(r) for r in given.find_many(texts, n=4)]
		pooled.close()
		given.close()


def test_names_and_the_reference_surface():
	_, embeddings, _ = pc.toy_session()
	static = embeddings["static"]
	for agg, name in ((np.mean, "mean"), (np.min, "min"), (np.max, "max")):
		emb = AggregatedSpanEmbedding(static, agg)
		assert emb.name == f"aggregated-{name}-toy-static"
		assert emb.dimension == static.dimension == pc.STATIC_D and emb.token_embedding is static and emb.agg is agg
	assert AggregatedSpanEmbedding(static).name == "aggregated-mean-toy-static"                       # np.mean is the default
	assert AggregatedSpanEmbedding(embeddings["contextual"], np.max, agg_name="peak").name == "aggregated-peak-toy-contextual"
	emb = AggregatedSpanEmbedding(static, np.min)
	assert isinstance(emb, SpanEmbedding)
	sim = emb.to_sentence_sim()
	assert isinstance(sim, EmbeddedSpanSim) and sim.embedding is emb and sim.name == "EmbeddedSpanSim"
	assert isinstance(emb.to_sentence_sim(CosineSim()), EmbeddedSpanSim)
	assert "vk_corpus_append_pooled" in core.EXPORTS
	assert [core.pool_code(a) for a in (np.mean, np.min, np.max, "mean", "min", "max", 0, 1, 2)] == [0, 1, 2] * 3


def test_refusals():
	session, embeddings, _ = pc.toy_session()
	for agg in (np.median, np.sum, lambda v, axis: v[0], "mean", None):
		with pytest.raises(NotImplementedError, match=r"np\.mean, np\.min or np\.max"):
			AggregatedSpanEmbedding(embeddings["static"], agg)
	with pytest.raises(NotImplementedError, match=r"np\.mean, np\.min or np\.max"):
		AggregatedSpanEmbedding(embeddings["static"], np.median, agg_name="median")             # a name does not make an aggregate
	with pytest.raises(NotImplementedError, match=r"np\.mean, np\.min or np\.max"):
		core.pool_code(np.median)
	# the span index computes the cosine: EmbeddedSpanSim keeps its refusal
	emb = AggregatedSpanEmbedding(embeddings["static"], np.mean)
	with pytest.raises(NotImplementedError, match="CosineSim"):
		session.partition("sentence").index(emb.to_sentence_sim(PNormDistance(2)), corpus_factory=Recording)
	with pytest.raises(TypeError):
		emb.to_sentence_sim("cosine")


@pytest.mark.parametrize("embedding", ["static", "contextual"])
def test_encode_is_the_numpy_aggregate_of_the_querys_token_vectors(embedding):
	_, embeddings, texts = pc.toy_session()
	token_embedding = embeddings[embedding]
	for agg in (np.mean, np.min, np.max):
		emb = AggregatedSpanEmbedding(token_embedding, agg)
		got = emb.encode(texts + [""])
		assert got.shape == (len(texts) + 1, token_embedding.dimension) and got.dtype == np.float32
		for row, text in zip(got, texts):
			want = agg(token_embedding.encode_tokens(text.split()).unmodified, axis=0)
			assert np.array_equal(row.view(np.uint32), want.astype(np.float32).view(np.uint32)), (embedding, agg, text)
		assert np.isnan(got[-1]).all()                                                              # no tokens: the reference's NaN row
	# the index hands its tokenizer on: the one call Query makes (nlp, dicts included)
	nlp = lambda text: [dict(text=t.lower(), pos="X", tag="x") for t in text.split("|")]
	bound = AggregatedSpanEmbedding(token_embedding, np.max).with_nlp(nlp)
	want = np.max(token_embedding.encode_tokens(["w1", "w2", "unseen"]).unmodified, axis=0)
	assert np.array_equal(bound.encode(["W1|w2|unseen"])[0], want)


def test_the_index_binds_its_tokenizer():
	session, embeddings, _ = pc.toy_session()
	seen = []

	def nlp(text):
		seen.append(text)
		return text.split()
	emb = AggregatedSpanEmbedding(embeddings["static"], np.mean)
	Recording.log = []
	index = session.partition("sentence").index(emb.to_sentence_sim(), nlp=nlp, corpus_factory=Recording)
	try:
		assert len(index.find("w1 w2 w3", n=2)) >= 1 and seen == ["w1 w2 w3"]
		assert emb.encode(["w1"]).shape == (1, pc.STATIC_D) and seen == ["w1 w2 w3"]                # the caller's embedding is as it was
	finally:
		index.close()
