"""Saliency: keyword signals per slice, smoothed over a document's neighbouring slices, averaged into one multiplicative boost per
slice -- the classes of vectorian/saliency.py with the same names, constructor arguments and meaning, restated for this project as
kernel.py and modifier.py restate theirs.  `HipBruteForceIndex(partition, sim, saliency=Saliency(...))` compiles the booster ON THE
DEVICE (vk_signal_keywords / vk_signal_filter / vk_corpus_set_saliency; vectorian_amd/csrc/vk_saliency_host.h states every cell) and
keeps it resident: queries then carry no boost array.

What the device computes, per document and in this order:
  * KeywordSignal: per slice -- window i of a document starts at span i * step and covers `size` spans, fewer at the end, as
    HipBruteForceIndex enumerates them -- the tokens whose vocabulary id is in the keyword set, float32(min(count, max_count)) /
    max_count.  The set is resolved once, here, against the session's vocabulary: a keyword outside it is dropped; with same= the
    predicate runs once per vocabulary entry.  The device only ever sees ids.
  * MaxFilter(width): scipy.ndimage.maximum_filter(x, size=width), one dimension, mode reflect, origin 0.
  * ConvFilter(pulse): np.convolve(x, pulse / sum(pulse), mode="same") in float64 where the pulse is no longer than the document, else x
    unchanged; GaussFilter(width, fc): the envelope of scipy.signal.gausspulse over linspace(-1, 1, width), restated in numpy (scipy is
    no dependency of the package; tests/test_saliency_py.py holds the restatement against scipy).
  * every signal is a float32 array before it is averaged; a filter's result is rounded to float32 where it is stored (upstream keeps
    the float64 of a convolution until the signal ends: a filter AFTER a convolution sees the rounded values here).
  * Saliency: np.average([ones, s_1 .. s_m], axis=0, weights=[1 - strength] + (w / sum(w) * strength)) in float64, rounded to float32
    once.  Without a signal the boost is all ones.

The filters' __call__ are host restatements of the same arithmetic in numpy, for a caller who wants a filter's answer on an array; the
index never calls them."""

import numpy as np

from vectorian_amd import core

# gausspulse's defaults (scipy.signal.gausspulse(t, fc, bw=0.5, bwr=-6, retenv=True)): the envelope is exp(-a t^2) with
# a = -(pi fc bw)^2 / (4 ln(10^(bwr / 20)))
_GAUSS_BW, _GAUSS_BWR = 0.5, -6


def gauss_envelope(t, fc=1):
	"""the envelope scipy.signal.gausspulse(t, fc=fc, retenv=True) returns, in numpy"""
	if fc < 0:
		raise ValueError(f"Center frequency (fc={fc:.2f}) must be >=0.")
	ref = pow(10.0, _GAUSS_BWR / 20.0)
	a = -(np.pi * fc * _GAUSS_BW) ** 2 / (4.0 * np.log(ref))
	t = np.asarray(t)
	return np.exp(-a * t * t)


class Filter:
	def __call__(self, x):
		raise NotImplementedError()

	def _device_filter(self):
		"""(core.VK_SIGNAL_FILTER_* kind, width, float64 pulse or None): what vk_signal_filter runs"""
		raise NotImplementedError(f"{type(self).__name__}: the device runs MaxFilter, ConvFilter and GaussFilter; a signal is smoothed there, "
			"not on the host")


class ConvFilter(Filter):
	def __init__(self, pulse):
		pulse = np.asarray(pulse)
		self._pulse = pulse / np.sum(pulse)

	def __call__(self, x):
		if self._pulse.shape[0] <= x.shape[0]:
			return np.convolve(x, self._pulse, mode='same')
		return x

	def _device_filter(self):
		if type(self).__call__ is not ConvFilter.__call__:
			return Filter._device_filter(self)
		pulse = np.ascontiguousarray(self._pulse, dtype=np.float64)
		if pulse.ndim != 1 or not 1 <= len(pulse) <= 4096 or not np.isfinite(pulse).all():
			raise NotImplementedError(f"{type(self).__name__}: a pulse of 1 .. 4096 finite taps")
		return core.VK_SIGNAL_FILTER_CONV, len(pulse), pulse


class GaussFilter(ConvFilter):
	def __init__(self, width, fc=1):
		t = np.linspace(-1, 1, width, endpoint=True)
		super().__init__(gauss_envelope(t, fc=fc))


class MaxFilter(Filter):
	def __init__(self, width):
		self._size = width

	def __call__(self, x):
		x = np.asarray(x)
		n, w = x.shape[0], int(self._size)
		if n == 0:
			return x
		left = w // 2   # the window of output i: inputs i - w // 2 .. i - w // 2 + w - 1, reflected about the edges
		padded = np.pad(x, (left, w - 1 - left), mode="symmetric")
		return np.lib.stride_tricks.sliding_window_view(padded, w).max(axis=1)

	def _device_filter(self):
		if type(self).__call__ is not MaxFilter.__call__:
			return Filter._device_filter(self)
		w = int(self._size)
		if w != self._size or not 1 <= w <= 4096:
			raise NotImplementedError(f"MaxFilter({self._size}): a width of 1 .. 4096 slices")
		return core.VK_SIGNAL_FILTER_MAX, w, None


class Signal:
	_filters = {
		'gauss': GaussFilter,
		'max': MaxFilter
	}

	def smoothed(self, width, method="max"):
		return SmoothedSignal(self, Signal._filters[method](width))

	def _compile(self, target, slot):
		"""leaves this signal in `slot` of target.corpus (a _CompileTarget)"""
		raise NotImplementedError(f"{type(self).__name__}: the device compiles KeywordSignal, CustomSignal and their smoothed forms")


class SmoothedSignal(Signal):
	def __init__(self, base, filter_):
		self._base = base
		self._filter = filter_

	def _compile(self, target, slot):
		kind, width, pulse = self._filter._device_filter()
		self._base._compile(target, slot)
		target.corpus.signal_filter(slot, kind, width, target.doc_off, pulse=pulse)


class CustomSignal(Signal):
	def spans_to_signal(self, spans):
		"""spans: the slices of ONE document, each a list of tokens with a `.text`; returns one value in [0, 1] per slice"""
		raise NotImplementedError()

	def _compile(self, target, slot):
		parts = []
		for spans in target.document_spans():
			signal = np.asarray(self.spans_to_signal(spans))
			if signal.shape != (len(spans),):
				raise ValueError(f"{type(self).__name__}.spans_to_signal: one value per span, got {signal.shape} for {len(spans)} spans")
			if len(spans):
				assert np.max(signal) <= 1
				assert np.min(signal) >= 0
			parts.append(signal.astype(np.float32))
		values = np.concatenate(parts) if parts else np.zeros(0, np.float32)
		target.corpus.signal_set(slot, values)


class KeywordSignal(CustomSignal):
	def __init__(self, *keywords, max_count=1, same=None):
		self._keywords = set(keywords)
		self._max_count = max_count
		self._same = same

	def _check(self, x):
		if self._same is None:
			return x in self._keywords
		for y in self._keywords:
			if self._same(x, y):
				return True
		return False

	def keyword_ids(self, vocab):
		"""the ids of the session vocabulary's entries that are keywords (int32, ascending): a keyword outside the vocabulary is
		dropped; with same= every vocabulary entry is asked once"""
		if self._same is None:
			ids = {vocab.token_to_id(k) for k in self._keywords}
			ids.discard(-1)
		else:
			ids = {i for i, token in enumerate(vocab.tokens) if self._check(token)}
		return np.array(sorted(ids), dtype=np.int32)

	def spans_to_signal(self, spans):
		"""the host's statement of the same signal (upstream's KeywordSignal.spans_to_signal); the index counts on the device"""
		w = np.zeros((len(spans),), dtype=np.float32)
		for i, span in enumerate(spans):
			w[i] = sum(1 for token in span if self._check(token.text))
		w = np.minimum(w, self._max_count)
		return w / self._max_count

	def _compile(self, target, slot):
		if type(self).spans_to_signal is not KeywordSignal.spans_to_signal:
			return CustomSignal._compile(self, target, slot)   # a subclass that counts its own way is a CustomSignal
		max_count = int(self._max_count)
		if max_count != self._max_count or max_count < 1:
			raise NotImplementedError(f"KeywordSignal(max_count={self._max_count}): a whole number >= 1")
		target.corpus.signal_keywords(slot, self.keyword_ids(target.vocab), max_count=max_count, token_ids=target.token_ids,
			vocab_size=max(1, target.vocab.size))


class _SpanToken:
	"""a token of a span as CustomSignal.spans_to_signal sees it"""
	__slots__ = ("text",)

	def __init__(self, text):
		self.text = text


class _CompileTarget:
	"""what a signal needs of the index it is compiled for: the handle, the session's vocabulary, the documents' offsets into the
	slices, and -- for a handle that keeps no token ids (contextual embeddings) -- the ids of every token"""

	def __init__(self, corpus, session, partition, doc_off, token_ids):
		self.corpus, self.vocab, self.doc_off, self.token_ids = corpus, session.vocab, doc_off, token_ids
		self._session, self._partition = session, partition

	def document_spans(self):
		level, size, step = self._partition.level, self._partition.window_size, self._partition.window_step
		for doc in self._session.documents:
			yield [[_SpanToken(t) for t in doc.span_tokens(level, sid, size)] for sid in range(0, doc.n_spans(level), step)]


class Saliency:
	def __init__(self, strength=0.5):
		self._signals = []
		self._w = []
		self._strength = strength
		if self._strength < 0 or self._strength > 1:
			raise ValueError(f"strength has illegal value {strength}")

	def add_signal(self, signal: Signal, weight: float = 1.0):
		self._signals.append(signal)
		self._w.append(weight)

	def weights(self):
		"""the weights of np.average over [ones, s_1 .. s_m] (upstream's Saliency.compile), float64"""
		if not self._signals:
			return np.array([1.0])
		w_sum = np.sum(self._w)
		normal_w = np.array(self._w) / w_sum
		return np.array([1 - self._strength] + (normal_w * self._strength).tolist(), dtype=np.float64)

	def compile(self, corpus, session, partition, doc_off, token_ids=None):
		"""compiles the booster on the device into `corpus` (a finalized core.Corpus over the partition's slices), where it stays
		resident; returns it, float32 [n_slices].  doc_off: [n_docs + 1] offsets of the documents into the slices; token_ids: the
		vocabulary id of every token, for a handle that keeps none"""
		if not hasattr(corpus, "set_saliency"):   # a capability of the backend: core.Corpus has it
			raise NotImplementedError("Saliency: this backend compiles no boosters; pass the boost as an array")
		if len(self._signals) > core.VK_MAX_SIGNALS:
			raise NotImplementedError(f"Saliency: {len(self._signals)} signals; the device averages at most {core.VK_MAX_SIGNALS}")
		weights = self.weights()
		if not np.isfinite(weights).all() or (weights < 0).any() or not weights.sum() > 0:
			raise ValueError(f"Saliency: weights must be finite, not negative and not all 0, got {list(self._w)}")
		target = _CompileTarget(corpus, session, partition, np.ascontiguousarray(doc_off, dtype=np.int64), token_ids)
		for slot, signal in enumerate(self._signals):
			signal._compile(target, slot)
		return corpus.set_saliency(np.arange(len(self._signals), dtype=np.int32), weights)
