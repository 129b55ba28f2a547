"""CPU tier: how a Saliency reaches the backend.  HipBruteForceIndex compiles it into the corpus it creates -- after finalize: per
signal the keyword / set call, then its filters, then one set_saliency -- and queries with boost=None; an array takes the path it
always took (no call but the query's own boost=); a sharded index refuses a Saliency by name.  The C-ABI exports the entry points and
refuses a null handle without touching a device."""

import ctypes as C

import numpy as np
import pytest

import saliency_cases as sc
from fake_backend import OracleCorpus
from saliency_backend import RecordingSaliencyCorpus
from test_host_api import toy_session
from vectorian_amd import alignment, core
from vectorian_amd.saliency import CustomSignal, KeywordSignal, Saliency
from vectorian_amd.sim import CosineSim, EmbeddingTokenSim, OptimizedSpanSim


def span_sim(emb):
	return OptimizedSpanSim(EmbeddingTokenSim(emb, CosineSim()), alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5)))


class _EverySecond(CustomSignal):
	def spans_to_signal(self, spans):
		return np.array([0.25 * (i % 2) for i in range(len(spans))])


def _saliency():
	s = Saliency(strength=0.6)
	s.add_signal(KeywordSignal("w1", "w3", "w7", "nowhere", max_count=2).smoothed(3), weight=2)
	s.add_signal(KeywordSignal("w2", "w5").smoothed(5, method="gauss"))
	s.add_signal(_EverySecond(), weight=0.5)
	return s


def test_a_saliency_is_compiled_in_order_and_queries_pass_no_boost():
	session, emb, words, rng = toy_session(n_docs=3, sents_per_doc=9, V=60, d=16)
	part = session.partition("sentence", 3, 2)   # windows of 3 sentences by 2
	index = part.index(span_sim(emb), saliency=_saliency(), corpus_factory=RecordingSaliencyCorpus)
	calls = index.corpus.calls
	assert [c[0] for c in calls] == ["finalize", "signal_keywords", "signal_filter", "signal_keywords", "signal_filter", "signal_set", "set_saliency"]
	n_slices = index.n_slices
	assert n_slices == 3 * 5
	doc_off = np.array([0, 5, 10, 15])
	vocab = session.vocab
	# signal 0: ids of the keywords in the vocabulary, max_count, the resident ids (static layout: none passed)
	_, slot, ids, max_count, token_ids, V = calls[1]
	assert slot == 0 and ids.tolist() == sorted(vocab.token_to_id(w) for w in ("w1", "w3", "w7")) and max_count == 2 and token_ids is None and V == vocab.size
	assert calls[2][1:4] == (0, core.VK_SIGNAL_FILTER_MAX, 3) and np.array_equal(calls[2][4], doc_off) and calls[2][5] is None
	assert calls[3][1] == 1 and calls[3][2].tolist() == sorted(vocab.token_to_id(w) for w in ("w2", "w5")) and calls[3][3] == 1
	assert calls[4][1:4] == (1, core.VK_SIGNAL_FILTER_CONV, 5) and np.array_equal(calls[4][4], doc_off)
	assert calls[4][5].dtype == np.float64 and np.array_equal(calls[4][5], sc.normalized(sc.gauss_pulse(5)))
	assert calls[5][1] == 2 and np.array_equal(calls[5][2], np.tile(np.array([0, 0.25, 0, 0.25, 0], np.float32), 3))
	assert calls[6][1].tolist() == [0, 1, 2] and np.array_equal(calls[6][2], np.array(sc.saliency_weights([2, 1.0, 0.5], 0.6)))
	# the booster: the restatement's, read-only
	ids_all = np.concatenate([session.doc_token_ids(i) for i in range(3)])
	k0 = sc.per_document(lambda x: sc.max_filter(x, 3), sc.keyword_signal(ids_all, index._slice_start, index._slice_end, calls[1][2], 2), doc_off)
	k1 = sc.per_document(lambda x: sc.conv_filter(x, calls[4][5]), sc.keyword_signal(ids_all, index._slice_start, index._slice_end, calls[3][2], 1), doc_off)
	want = sc.average([k0, k1, calls[5][2]], calls[6][2], n_slices)
	assert index.boost.dtype == np.float32 and np.array_equal(index.boost, want) and not index.boost.flags.writeable
	assert len(np.unique(want)) > 3   # the signals fire
	# queries pass no boost; their matches are those of an index given the array
	doc = session.documents[1]
	text = " ".join(doc.tokens[5:10])
	res = index.find(text, n=5)
	assert [c[0] for c in calls[7:]] == ["query"] and calls[7][1] is None
	by_array = part.index(span_sim(emb), saliency=want, corpus_factory=RecordingSaliencyCorpus)
	ref = by_array.find(text, n=5)
	assert [(m.doc_index, m.slice_id, m.score) for m in res] == [(m.doc_index, m.slice_id, m.score) for m in ref] and len(res) == 5
	plain = part.index(span_sim(emb), corpus_factory=RecordingSaliencyCorpus).find(text, n=5)
	assert [m.score for m in plain] != [m.score for m in res]   # the boost shows
	# find_many: the further handles share the resident booster
	many = index.find_many([text, text], n=5, batch=False)
	assert all([(m.doc_index, m.slice_id, m.score) for m in r] == [(m.doc_index, m.slice_id, m.score) for m in ref] for r in many)
	assert all(c[0] == "query" and c[1] is None for c in calls[8:])


def test_an_array_makes_the_calls_it_always_made():
	session, emb, words, rng = toy_session(n_docs=3, sents_per_doc=9, V=60, d=16)
	part = session.partition("sentence")
	boost = (1 + 0.1 * np.arange(27)).astype(np.float64)   # any array-like, converted once
	index = part.index(span_sim(emb), saliency=boost, corpus_factory=RecordingSaliencyCorpus)
	assert [c[0] for c in index.corpus.calls] == ["finalize"]
	index.find(" ".join(session.documents[0].tokens[:4]), n=3)
	assert [c[0] for c in index.corpus.calls] == ["finalize", "query"]
	assert index.corpus.calls[1][1].dtype == np.float32 and np.array_equal(index.corpus.calls[1][1], boost.astype(np.float32))
	assert np.array_equal(index.boost, boost.astype(np.float32)) and not index.boost.flags.writeable
	assert part.index(span_sim(emb), corpus_factory=RecordingSaliencyCorpus).boost is None
	with pytest.raises(ValueError):
		part.index(span_sim(emb), saliency=boost[:5], corpus_factory=RecordingSaliencyCorpus)


def test_a_sharded_index_refuses_a_saliency_by_name_and_keeps_arrays():
	session, emb, words, rng = toy_session(n_docs=3, sents_per_doc=9, V=60, d=16)
	part = session.partition("sentence")
	with pytest.raises(NotImplementedError) as e:
		part.index(span_sim(emb), saliency=_saliency(), shard=(0, 2), corpus_factory=RecordingSaliencyCorpus)
	assert "Saliency on a sharded index" in str(e.value) and "shard" in str(e.value)
	index = part.index(span_sim(emb), saliency=np.ones(27, np.float32), shard=(0, 2), corpus_factory=RecordingSaliencyCorpus)
	assert [c[0] for c in index.corpus.calls] == ["finalize"]


def test_a_backend_without_the_methods_refuses_by_capability():
	session, emb, words, rng = toy_session(n_docs=2, sents_per_doc=5, V=60, d=16)
	with pytest.raises(NotImplementedError) as e:
		session.partition("sentence").index(span_sim(emb), saliency=_saliency(), corpus_factory=OracleCorpus)
	assert "compiles no boosters" in str(e.value)


def test_the_entry_points_are_exported_and_refuse_a_null_handle():
	lib = core.lib()
	names = ("vk_signal_keywords", "vk_signal_set", "vk_signal_filter", "vk_corpus_set_saliency", "vk_corpus_clear_saliency")
	for name in names:
		assert name in core.EXPORTS and hasattr(lib, name), name
	ids, vals, w, off = np.zeros(2, np.int32), np.ones(2, np.float32), np.ones(3, np.float64), np.zeros(2, np.int64)
	p = lambda a: a.ctypes.data_as(C.c_void_p)
	assert lib.vk_signal_keywords(None, 0, p(ids), 2, 1, None, 10) == core.VK_ERR_INVALID and b"null" in lib.vk_last_error()
	assert lib.vk_signal_set(None, 0, p(vals)) == core.VK_ERR_INVALID
	assert lib.vk_signal_filter(None, 0, core.VK_SIGNAL_FILTER_MAX, 3, None, p(off), 1) == core.VK_ERR_INVALID
	assert lib.vk_corpus_set_saliency(None, p(ids), p(w), 2, None) == core.VK_ERR_INVALID
	assert lib.vk_corpus_clear_saliency(None) == core.VK_ERR_INVALID
	assert core.VK_MAX_SIGNALS == 8 and (core.VK_SIGNAL_FILTER_MAX, core.VK_SIGNAL_FILTER_CONV) == (0, 1)
