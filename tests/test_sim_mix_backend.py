"""CPU tier: how a token similarity combinator reaches the backend.  HipBruteForceIndex hands MixedTokenSimilarity /
MaximumTokenSimilarity / MinimumTokenSimilarity over static embeddings to the corpus it creates -- set_sim_mix, then per operand
set_sim_operand / append_operand_vectors, before finalize; operand 0's source and chain through the old setters; the query's rows
under the other operands' embeddings with every find -- and refuses, by name, what the device does not compute.  The Python classes
compute what the reference's compute, `MinimumTokenSimilarity` the cell-wise MAXIMUM included.  The conditions on the inputs of the GPU
tier (tests/test_gpu_token_sim_mix.py) are asserted here, where the reference side needs no GPU.  The C-ABI exports the entry points
and refuses a null handle without touching a device."""

import ctypes as C

import numpy as np
import pytest

import sim_mix_cases as mc
import sim_ops_cases as sc
from oracle import vk_oracle as vo
from sim_mix_backend import MixOracleCorpus, MixRecordingCorpus
from test_host_api import toy_session
from vectorian_amd import alignment, core
from vectorian_amd.corpus import Document
from vectorian_amd.embedding import ContextualEmbedding, StaticEmbedding
from vectorian_amd.modifier import (MaximumTokenSimilarity, MinimumTokenSimilarity, MixedTokenSimilarity, TokenSimilarityModifier,
	UnaryTokenSimilarityModifier)
from vectorian_amd.session import Session
from vectorian_amd.sim import (Bias, CosineSim, DistanceToSimilarity, EmbeddingTokenSim, ModifiedVectorSim, OptimizedSpanSim, PNormDistance, Scale,
	Threshold, TokenSim)
from vectorian_amd import sim as sim_module


def two_embeddings(d2=24, **kw):
	"""toy_session's session with a second static embedding over the same words"""
	session, emb, words, rng = toy_session(**kw)
	E2 = np.random.default_rng(99).standard_normal((len(words), d2)).astype(np.float32)
	emb2 = StaticEmbedding(f"other-{d2}", words, E2)
	session = Session(session.documents, embeddings=[emb, emb2])
	return session, emb, emb2, words


def _span(token_sim, optimizer=None):
	return OptimizedSpanSim(token_sim, optimizer or alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5)))


def test_the_combinator_reaches_the_corpus_before_finalize_and_the_query_operands_with_every_find():
	session, emb, emb2, words = two_embeddings(n_docs=3, sents_per_doc=20, V=300, d=32)
	first = EmbeddingTokenSim(emb, ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5)))
	second = EmbeddingTokenSim(emb2, ModifiedVectorSim(PNormDistance(2), Scale(0.07), DistanceToSimilarity()))
	mixed = MixedTokenSimilarity([first, second], [2, 1])
	index = session.partition("sentence").index(_span(mixed), corpus_factory=MixRecordingCorpus)
	calls = index.corpus.calls
	assert [c[0] for c in calls] == ["set_sim_mix", "set_sim_operand", "append_operand_vectors", "append_vectors", "set_sim_ops", "finalize"]
	_, kind, n, weights = calls[0]
	assert kind == core.VK_SIMMIX_AVERAGE and n == 2
	assert isinstance(weights, np.ndarray) and weights.dtype == np.float64 and list(weights) == [2.0, 1.0]   # int weights arrive as float64
	_, i, d, source, ops = calls[1]
	assert (i, d) == (1, 24) and source == (core.VK_SIMSRC_PNORM, np.float32(2)) and isinstance(source[1], np.float32)
	assert ops == [(core.VK_SIMOP_SCALE, np.float32(0.07)), (core.VK_SIMOP_ONE_MINUS, np.float32(0))]
	assert calls[2][1:] == (1, (session.vocab.size, 24), np.float32, True)
	assert (index.corpus.operand_rows[1][0] == emb2.encode_tokens(session.vocab.tokens).unmodified).all()   # the unmodified rows
	assert calls[4][1] == [(core.VK_SIMOP_BIAS, np.float32(1)), (core.VK_SIMOP_SCALE, np.float32(0.5))]      # operand 0: the old setter
	assert index.metric_name == mixed.name == f"({2 / 3} * {first.name} + {1 / 3} * {second.name})"
	# every find brings the query's rows under the other operand's embedding
	doc = session.documents[1]
	st = doc.spans["sentence"]["start"][4]
	tokens = doc.tokens[st:st + 5]
	index.find(" ".join(tokens), n=5)
	index.find(" ".join(tokens[:3]), n=5)
	assert [len(q) for q in index.corpus.query_operands] == [1, 1]
	a, b = index.corpus.query_operands
	assert a[0].shape == (5, 24) and b[0].shape == (3, 24) and a[0].dtype == np.float32
	assert (a[0] == emb2.encode_tokens(tokens).unmodified).all()
	# MAXIMUM: no weights; three operands in order
	third = EmbeddingTokenSim(emb, CosineSim())
	for cls in (MaximumTokenSimilarity, MinimumTokenSimilarity):
		index = session.partition("sentence").index(_span(cls([first, second, third])), corpus_factory=MixRecordingCorpus)
		calls = index.corpus.calls
		assert [c[0] for c in calls] == ["set_sim_mix", "set_sim_operand", "append_operand_vectors", "set_sim_operand", "append_operand_vectors",
			"append_vectors", "set_sim_ops", "finalize"]
		assert calls[0][1:] == (core.VK_SIMMIX_MAXIMUM, 3, None)   # "minimum" runs what upstream's __call__ computes: the maximum
		assert calls[3][1:] == (2, 32, None, [])
	assert index.metric_name == f"minimum({first.name}, {second.name}, {third.name})"
	# a plain cosine index makes none of these calls, and its queries carry no operand rows
	plain = session.partition("sentence").index(_span(EmbeddingTokenSim(emb, CosineSim())), corpus_factory=MixRecordingCorpus)
	assert [c[0] for c in plain.corpus.calls] == ["append_vectors", "finalize"]
	plain.find(" ".join(tokens), n=5)
	assert plain.corpus.query_operands == [None]


def test_find_and_find_many_under_a_combinator_on_the_double():
	session, emb, emb2, words = two_embeddings(n_docs=3, sents_per_doc=20, V=300, d=32)
	a = sc.chain("a")
	mixed = MixedTokenSimilarity([EmbeddingTokenSim(emb, ModifiedVectorSim(CosineSim(), *a)), EmbeddingTokenSim(emb2, ModifiedVectorSim(CosineSim(), *a))], [0.3, 0.7])
	index = session.partition("sentence").index(_span(mixed), corpus_factory=MixOracleCorpus)
	doc = session.documents[1]
	st = doc.spans["sentence"]["start"][4]
	text = " ".join(doc.tokens[st:st + 5])
	res = index.find(text, n=5)
	assert res[0].doc_index == 1 and res[0].slice_id == 4 and abs(res[0].score - 1.0) < 1e-6
	assert [m.score for m in res] == sorted((m.score for m in res), reverse=True) and res[4].score > 0.55
	many = index.find_many([text, " ".join(doc.tokens[st:st + 3])], n=5)
	assert [(m.doc_index, m.slice_id, m.score) for m in many[0]] == [(m.doc_index, m.slice_id, m.score) for m in res]
	alone = session.partition("sentence").index(_span(mixed.operands[0]), corpus_factory=MixOracleCorpus)
	assert [m.score for m in alone.find(text, n=5)][1:] != [m.score for m in res][1:]


def _dicts(tables):
	return [{"similarity": t, "magnitudes": np.full(t.shape[0], 1.0 + i, np.float32)} for i, t in enumerate(tables)]


def test_the_classes_compute_what_the_references_compute():
	rng = np.random.default_rng(3)
	S = [np.clip(rng.uniform(-0.2, 1.1, size=(6, 4)), 0, 1).astype(np.float32) for _ in range(3)]
	S[1][0, 0] = S[0][0, 0]   # equal cells: the first operand's, the same float
	for w in ([0.2, 0.5, 0.3], [1, 2, 3], [1.5, 0, 0.25]):
		out = {"similarity": np.empty((6, 4), np.float32), "magnitudes": np.empty(6, np.float32)}
		MixedTokenSimilarity([None] * 3, w)(_dicts(S), out)
		want = ((S[0].astype(np.float64) * w[0] + S[1].astype(np.float64) * w[1]) + S[2].astype(np.float64) * w[2]) / ((float(w[0]) + w[1]) + w[2])
		assert (out["similarity"] == want.astype(np.float32)).all()
		assert np.allclose(out["magnitudes"], (1 * w[0] + 2 * w[1] + 3 * w[2]) / sum(w))   # magnitudes are averaged with the same weights
	for cls in (MaximumTokenSimilarity, MinimumTokenSimilarity):
		out = {"similarity": np.empty((6, 4), np.float32)}
		cls([None] * 3)(_dicts(S), out)
		assert (out["similarity"] == np.maximum.reduce(S)).all(), cls   # MinimumTokenSimilarity returns the cell-wise maximum, as upstream
	assert not (np.maximum.reduce(S) == np.minimum.reduce(S)).all()
	out = {"similarity": np.empty((6, 4), np.float32), "magnitudes": np.empty(6, np.float32)}
	UnaryTokenSimilarityModifier(None, [Bias(1), Scale(2)])(_dicts(S[:1]), out)
	assert (out["similarity"] == (S[0] + np.float32(1)) * np.float32(2)).all() and (out["similarity"] > 1).any()   # leaves [0, 1] unclipped
	assert (out["magnitudes"] == 1).all()


def test_names_operands_embeddings_and_the_re_export():
	session, emb, emb2, words = two_embeddings(n_docs=2, sents_per_doc=5, V=100, d=16)
	x, y = EmbeddingTokenSim(emb, CosineSim()), EmbeddingTokenSim(emb2, ModifiedVectorSim(CosineSim(), Threshold(0.2)))
	mixed = MixedTokenSimilarity([x, y], [1, 3])
	assert mixed.name == f"(0.25 * {x.name} + 0.75 * {y.name})" and mixed.operands == [x, y] and mixed.embeddings == [emb, emb2] and mixed.is_modifier
	assert MaximumTokenSimilarity([x, y]).name == f"maximum({x.name}, {y.name})" and MinimumTokenSimilarity([x, y]).name == f"minimum({x.name}, {y.name})"
	unary = UnaryTokenSimilarityModifier(x, [Bias(1)])
	assert unary.name == f"({x.name} + 1)" and unary.operands == [x] and unary.embeddings == [emb]
	for name in ("TokenSimilarityModifier", "UnaryTokenSimilarityModifier", "MixedTokenSimilarity", "MaximumTokenSimilarity", "MinimumTokenSimilarity"):
		assert getattr(sim_module, name) is getattr(__import__("vectorian_amd.modifier", fromlist=[name]), name)
	assert issubclass(TokenSimilarityModifier, TokenSim)
	with pytest.raises(AttributeError):
		sim_module.NoSuchSimilarity


def test_what_stays_refused_says_which_case_it_is():
	session, emb, emb2, words = two_embeddings(n_docs=2, sents_per_doc=5, V=100, d=16)
	part = session.partition("sentence")
	x, y = EmbeddingTokenSim(emb, CosineSim()), EmbeddingTokenSim(emb2, CosineSim())

	def refused(sim, *words_in_message):
		with pytest.raises(NotImplementedError) as e:
			part.index(sim, corpus_factory=MixRecordingCorpus)
		for w in words_in_message:
			assert w in str(e.value), (w, str(e.value))
	refused(_span(UnaryTokenSimilarityModifier(x, [Bias(1)])), "UnaryTokenSimilarityModifier", "unclipped", "ModifiedVectorSim")
	refused(_span(MixedTokenSimilarity([x, MaximumTokenSimilarity([x, y])], [1, 1])), "nested", "MaximumTokenSimilarity")
	refused(_span(MaximumTokenSimilarity([x, UnaryTokenSimilarityModifier(y, [Bias(1)])])), "nested", "UnaryTokenSimilarityModifier")
	refused(_span(MaximumTokenSimilarity([x, y, x, y, x])), "5 operands", "2 to 4")
	refused(_span(MixedTokenSimilarity([x], [1])), "1 operands")
	refused(_span(MixedTokenSimilarity([x, y], [1, -1])), "not negative")
	refused(_span(MixedTokenSimilarity([x, y], [1, float("nan")])), "finite")
	refused(_span(MixedTokenSimilarity([x, y], [1, float("inf")])), "finite")
	refused(_span(MixedTokenSimilarity([x, y], [0, 0])), "sum to 0")
	refused(_span(MixedTokenSimilarity([x, y], [1, 2, 3])), "3 weights for 2 operands")
	for cls, args in ((MixedTokenSimilarity, ([1, 1],)), (MaximumTokenSimilarity, ()), (MinimumTokenSimilarity, ())):
		refused(_span(cls([x, y], *args), alignment.WordRotatorsDistance()), "WordRotatorsDistance", "magnitudes")
	# an operand's own similarity is refused as an index's is
	refused(_span(MaximumTokenSimilarity([x, EmbeddingTokenSim(emb2, ModifiedVectorSim(CosineSim(), *([Bias(0.1)] * 9)))])), "9 operators", "at most 8")

	class Mine(MixedTokenSimilarity):
		def __call__(self, operands, out):
			out["similarity"][:] = 0
	refused(_span(Mine([x, y], [1, 1])), "Mine", "ModifiedVectorSim")

	class Other(TokenSimilarityModifier):
		operands = [x, y]
	refused(_span(Other()), "Other", "token similarity modifiers", "ModifiedVectorSim")

	class Plain(TokenSim):   # a TokenSim that is none of ours
		is_modifier = True
	refused(OptimizedSpanSim(Plain()), "token similarity modifiers", "ModifiedVectorSim")
	# a contextual operand
	d = 16
	vecs = np.random.default_rng(0).standard_normal((100, d)).astype(np.float32)
	ctx = ContextualEmbedding("ctx", d, lambda tokens: np.stack([vecs[int(t[1:])] for t in tokens]))
	toks = [["w1", "w2", "w3"], ["w4", "w5"]]
	docs = [Document(toks, contextual_embeddings={"ctx": np.stack([vecs[int(t[1:])] for s in toks for t in s])})]
	static = StaticEmbedding("st", [f"w{i}" for i in range(100)], vecs)
	csession = Session(docs, embeddings=[static, ctx])
	with pytest.raises(NotImplementedError) as e:
		csession.index(_span(MaximumTokenSimilarity([EmbeddingTokenSim(static, CosineSim()), EmbeddingTokenSim(ctx, CosineSim())])), corpus_factory=MixRecordingCorpus)
	assert "static embeddings only" in str(e.value) and "ctx is contextual" in str(e.value)


# ---- the conditions on the inputs of the GPU tier

@pytest.mark.parametrize("case", sorted(mc.CASES))
def test_the_gpu_tiers_inputs_meet_their_conditions(case):
	"""per case of tests/test_gpu_token_sim_mix.py: a third of the combined table's cells inside (0, 1) and, under MAXIMUM, every
	operand the strict maximum in a fifth of them (sim_mix_cases.tables asserts both, for every query length); and for at least one
	query the reference's winners under the combinator are not its winners under operand 0 alone"""
	corpus, name, mix = mc.case(case)
	ops_of = mc.operands(name, corpus.dims)
	differ = 0
	for len_t in mc.QUERY_LENGTHS:
		q_ids, Qs = corpus.query(len_t, seed=mc.QUERY_SEED)
		T, each = mc.tables(vo, corpus, q_ids, Qs, ops_of, mix)
		kw = dict(layout=vo.LAYOUT_CONTEXTUAL, d=corpus.dims[0], sent_off=corpus.off, Q=vo.normalize_rows_bf16(Qs[0])[0], locality=0, gap_s=0.1, gap_t=0.05,
			max_matches=9, min_score=0.0)
		both, alone = vo.find(S_rows=[T[corpus.ids]], **kw), vo.find(S_rows=[each[0][corpus.ids]], **kw)
		differ += list(both["sentence"]) != list(alone["sentence"])
	assert differ >= 1


def test_the_entry_points_are_exported_and_refuse_a_null_handle():
	lib = core.lib()
	names = ("vk_corpus_set_sim_mix", "vk_corpus_set_sim_operand", "vk_corpus_append_operand_vectors", "vk_corpus_set_query_operand")
	for name in names:
		assert name in core.EXPORTS and hasattr(lib, name)
	w = np.ones(2, np.float64)
	rows = np.zeros((2, 4), np.float32)
	ptr = lambda a: a.ctypes.data_as(C.c_void_p)
	assert lib.vk_corpus_set_sim_mix(None, core.VK_SIMMIX_AVERAGE, 2, ptr(w)) == core.VK_ERR_INVALID and b"null" in lib.vk_last_error()
	assert lib.vk_corpus_set_sim_operand(None, 1, 4, 0, 0.0, None, None, 0) == core.VK_ERR_INVALID
	assert lib.vk_corpus_append_operand_vectors(None, 1, ptr(rows), 2, core.VK_F32, 1) == core.VK_ERR_INVALID
	assert lib.vk_corpus_set_query_operand(None, 1, ptr(rows), 2, core.VK_F32, 1) == core.VK_ERR_INVALID
	assert (core.VK_SIMMIX_NONE, core.VK_SIMMIX_AVERAGE, core.VK_SIMMIX_MAXIMUM) == (0, 1, 2) and core.VK_MAX_SIM_OPERANDS == 4 and lib.vk_abi_version() == 12
