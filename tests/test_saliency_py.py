"""CPU tier: vectorian_amd/saliency.py, the project's restatement of the reference's saliency classes -- what it computes on the host
before anything reaches a device: GaussFilter's pulse (held against scipy), the strength of a Saliency and its weights, the ids a
KeywordSignal resolves to, the range a CustomSignal must keep, and the host statements of the filters."""

import numpy as np
import pytest

import saliency_cases as sc
from saliency_backend import RecordingSaliencyCorpus
from test_host_api import toy_session
from vectorian_amd import core
from vectorian_amd.saliency import (ConvFilter, CustomSignal, Filter, GaussFilter, KeywordSignal, MaxFilter, Saliency, Signal, SmoothedSignal,
	gauss_envelope)
from vectorian_amd.session import Vocabulary


@pytest.mark.parametrize("fc", [1, 0.5, 2.5])
@pytest.mark.parametrize("width", [1, 2, 3, 4, 5, 8, 9, 31])
def test_the_gauss_pulse_is_scipys(width, fc):
	scipy_signal = pytest.importorskip("scipy.signal")
	t = np.linspace(-1, 1, width, endpoint=True)
	_, e = scipy_signal.gausspulse(t, fc=fc, retenv=True)
	assert np.array_equal(gauss_envelope(t, fc=fc), e)
	want = e / np.sum(e)
	got = GaussFilter(width, fc=fc)._pulse
	assert got.dtype == np.float64 and np.array_equal(got, want)
	kind, w, pulse = GaussFilter(width, fc=fc)._device_filter()
	assert (kind, w) == (core.VK_SIGNAL_FILTER_CONV, width) and np.array_equal(pulse, want)


def test_strength_is_validated_and_the_weights_are_upstreams():
	for bad in (-0.01, 1.01, 2, -1):
		with pytest.raises(ValueError) as e:
			Saliency(strength=bad)
		assert "strength has illegal value" in str(e.value)
	for ok in (0, 0.5, 1):
		Saliency(strength=ok)
	assert np.array_equal(Saliency().weights(), [1.0])   # no signal: all ones
	s = Saliency(strength=0.3)
	s.add_signal(KeywordSignal("a"))
	s.add_signal(KeywordSignal("b"), weight=3)
	s.add_signal(KeywordSignal("c"), weight=0.5)
	assert np.array_equal(s.weights(), np.array(sc.saliency_weights([1.0, 3, 0.5], 0.3), dtype=np.float64))


def test_keywords_resolve_to_ids_over_the_vocabulary():
	vocab = Vocabulary()
	for t in ["the", "Whale", "whale", "sea", "WHALE", "ship", "Sea"]:
		vocab.add(t)
	# exact: a keyword outside the vocabulary is dropped, one given twice counts once
	assert KeywordSignal("whale", "sea", "kraken", "whale").keyword_ids(vocab).tolist() == [2, 3]
	assert KeywordSignal("kraken").keyword_ids(vocab).tolist() == []
	# same=: the predicate runs once per vocabulary entry (and keyword), never per token of the corpus
	asked = []

	def same(x, y):
		asked.append(x)
		return x.lower() == y
	ids = KeywordSignal("whale", "sea", same=same, max_count=2).keyword_ids(vocab)
	assert ids.dtype == np.int32 and ids.tolist() == [1, 2, 3, 4, 6]
	assert set(asked) == set(vocab.tokens) and len(asked) <= 2 * vocab.size


def test_a_custom_signal_stays_in_range():
	session, emb, words, rng = toy_session(n_docs=2, sents_per_doc=6, V=50, d=16)
	part = session.partition("sentence")
	from test_saliency_backend import span_sim

	class Lengths(CustomSignal):
		def __init__(self, scale):
			self._scale = scale

		def spans_to_signal(self, spans):
			assert all(hasattr(t, "text") for span in spans for t in span)
			return np.array([len(span) / self._scale for span in spans])

	for scale, fine in ((40.0, True), (10.0, False), (-40.0, False)):
		s = Saliency()
		s.add_signal(Lengths(scale))
		if fine:
			index = part.index(span_sim(emb), saliency=s, corpus_factory=RecordingSaliencyCorpus)
			sent = [c for c in index.corpus.calls if c[0] == "signal_set"]
			assert len(sent) == 1 and sent[0][2].dtype == np.float32 and len(sent[0][2]) == 12
			assert np.array_equal(sent[0][2], ((index._slice_end - index._slice_start).astype(np.float64) / 40.0).astype(np.float32))
		else:
			with pytest.raises(AssertionError):
				part.index(span_sim(emb), saliency=s, corpus_factory=RecordingSaliencyCorpus)

	class TooFew(CustomSignal):
		def spans_to_signal(self, spans):
			return np.zeros(len(spans) + 1)
	s = Saliency()
	s.add_signal(TooFew())
	with pytest.raises(ValueError):
		part.index(span_sim(emb), saliency=s, corpus_factory=RecordingSaliencyCorpus)


def test_the_filters_on_the_host_state_the_same_arithmetic():
	"""Filter.__call__ for a caller's own arrays: MaxFilter == scipy's maximum_filter, ConvFilter == upstream's"""
	for name, kind, width, pulse, off, x, want in sc.filter_cases():
		f = MaxFilter(width) if kind == 0 else ConvFilter(pulse)
		got = sc.per_document(f, x, off)
		assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
	assert isinstance(KeywordSignal("a").smoothed(3), SmoothedSignal) and isinstance(KeywordSignal("a").smoothed(3)._filter, MaxFilter)
	assert isinstance(KeywordSignal("a").smoothed(5, method="gauss")._filter, GaussFilter)
	with pytest.raises(NotImplementedError):
		Filter()(np.zeros(3))


def test_what_the_device_does_not_compile_is_refused_by_name():
	class Mine(Filter):
		def __call__(self, x):
			return x * 0.5

	class Other(Signal):
		pass
	session, emb, words, rng = toy_session(n_docs=2, sents_per_doc=6, V=50, d=16)
	part = session.partition("sentence")
	from test_saliency_backend import span_sim
	for signal, word in ((SmoothedSignal(KeywordSignal("w1"), Mine()), "Mine"), (Other(), "Other"), (KeywordSignal("w1", max_count=0), "max_count"),
			(KeywordSignal("w1").smoothed(5000), "4096")):
		s = Saliency()
		s.add_signal(signal)
		with pytest.raises(NotImplementedError) as e:
			part.index(span_sim(emb), saliency=s, corpus_factory=RecordingSaliencyCorpus)
		assert word in str(e.value), str(e.value)
	s = Saliency()
	for k in range(core.VK_MAX_SIGNALS + 1):
		s.add_signal(KeywordSignal(f"w{k}"))
	with pytest.raises(NotImplementedError) as e:
		part.index(span_sim(emb), saliency=s, corpus_factory=RecordingSaliencyCorpus)
	assert "9 signals" in str(e.value)
